"""The packed winding cells of k_raster_fill and k_raster_rows (fill + 65536 * hull in one 32-bit integer per sample) at their limits.

What moves a cell, from the kernels (csrc/raster_edges.hip) and the binning that writes their lists (csrc/bin_edges.hip):
  * a boundary edge of the fill chain adds sigma * [Y g(p) + A] to the fill half, a hull edge the same to the hull half; Y g(p) + A takes
    the values -1, 0, 1 only (the three cases of A in k_raster_fill), so an edge entry moves ONE half by ONE at most;
  * a backdrop unit (codes 0 - 3) is +1 or -1 on one half — a tile that lies |b| deep inside a Shape holds |b| - 1 such entries;
  * a curve triangle adds or subtracts its accept bit: one, on the fill half;
  * a COVER entry folds in one unit of either backdrop, (f - 1) + (h - 1) * 65536 with f, h in 0 .. 2: one per half.
No entry moves a half by two. Additions are linear modulo 2^32 and the halves are only taken apart at covers, so a cell is exact while
|fill| and |hull| stay below 2^15, that is while a tile's list has fewer than 32 768 entries. The host hands the two kernels only frames
whose longest list ever measured is below GATE = 16 384 (api.hip, RasterParams::rows / fill_cells); between two measurements a list in
place can grow to its place's capacity, c + c / 2 + 64 with c <= 16 383: IN_PLACE_MAX = 24 638 entries, still below 32 768. That growth is
what the gate's margin is for, and test_growth_between_verified_passes draws it (a growth from 16 383 to 24 636 entries in one step is
drawn again the verified way on this build, so the packed kernels themselves are drawn up to 16 383 entries here; the per-sample kernels to 37 109).

The scenes are tests/packed_cells_model.py's stacks: the expected image is a count per sample, no oracle and no eps band. Families:
  deep   ONE Shape of K rectangles (one item, one cover): the fill half of a cell reaches +-K. Clockwise, all reversed (the fill half deeply
         negative, borrowing from the hull half) and mixed (the running count crosses 0 and multiples of 2^bits at the sample columns);
  many   K Shapes of one rectangle each (K covers, every cell back to zero K times), opaque and translucent colours in turn.
There is no third family: it was meant for an entry kind that moves a counter by two, and there is none.

Every case asserts the longest list (crh_debug_frame_counters word 3) and the kernel (crh_debug_frame_last_pass) it claims."""
import ctypes as C
import functools

import numpy as np
import pytest

from contrast_renderer_amd import Path, batch_from_shapes

import packed_cells_model as M
from test_ground_truth import GPU_PATHS, path_ran

GATE = 16384  # api.hip render_impl: `f->longest_list < 16384u` (p.rows, p.fill_cells, and again behind the verified pass' read-back)
LDS_SORT_MAX = {1: 8192, 4: 2048}  # raster_common.hpp kSortBytesMax / (4 bytes x wavefronts of a tile): longer lists are sorted in place


def place_capacity(c):
    """raster_params.hpp RasterParams::tile_base / api.hip launch_tile_bases: the place a list of c entries is given for the next pass."""
    return c + c // 2 + 64


IN_PLACE_MAX = place_capacity(GATE - 1)  # the longest list a packed kernel can be handed
assert IN_PLACE_MAX == 24638 and IN_PLACE_MAX < 32768

# Entries of the longest list under the edge formulation (k_bin_edges / k_bin_flat), measured once and asserted by every case:
#   deep: the K left edges + the Shape's COVER + the left edge of its hull, in every tile of column 1;
#   many: per Shape its left edge, its hull's left edge and its COVER; a filler (a rectangle over the whole of columns 1 - 3) its COVER only.
DEEP_EXTRA = 2
MANY_PER_SHAPE = 3


def deep_stack(variant, n, bits=8):
    k = n - DEEP_EXTRA
    if variant == "mixed":
        j = M.staggers(k + 16, M.stride_for(k))
        keep, signs = M.mixed_signs(j, bits)
        assert len(keep) >= k
        j, signs = j[keep][:k], signs[:k]
    else:
        j = M.staggers(k, M.stride_for(k))
        signs = np.full(k, 1 if variant == "cw" else -1)
    return [M.Stack(j, signs)]


def many_stacks(n):
    k, fillers = n // MANY_PER_SHAPE, n % MANY_PER_SHAPE
    rng = np.random.RandomState(n)
    out = [M.Stack([1 + 2 * f], [1], (0.2 + 0.3 * f, 0.5, 0.9 - 0.3 * f, 1.0), shift=-16.0) for f in range(fillers)]  # at the bottom: nothing starts late behind them
    every = max(2, -(-k // 24))  # at most 24 translucent layers in all (the tolerance below allows 28 blends)
    for i, j in enumerate(M.staggers(k, M.stride_for(k))):
        rgb = rng.uniform(0.0, 1.0, 3)
        alpha = float(rng.uniform(0.2, 0.8)) if i % every == every // 2 else 1.0
        out.append(M.Stack([j], [1 if i % 3 else -1], (rgb[0], rgb[1], rgb[2], alpha)))
    return out


@functools.lru_cache(maxsize=2)
def _scene_of(family, n, bits):
    stacks = many_stacks(n) if family == "many" else deep_stack(family.split("-")[1], n, bits)
    return stacks, batch_of(stacks)


def scene_of(family, n, bits=8):
    """-> (stacks, path batch), built once per scene (only the mixed stack depends on the counter width)."""
    return _scene_of(family, n, bits if family == "deep-mixed" else 0)


def stacks_of(family, n, bits=8):
    return scene_of(family, n, bits)[0]


def batch_of(stacks):
    return batch_from_shapes([([], [Path.from_polygon(p) for p in st.polygons()]) for st in stacks])


def expected_bytes(stacks, msaa, bits, shifts=None):
    """-> (expected [64, 64, 4] float64 in [0, 1], tolerance): an exact image for opaque white stacks, else the RGBA8 tolerance of
    colour-over-rgba8-msaa4 (test_ground_truth.py): half a unit of the one rounding to unorm8 + 2^-24 per f32 operation on a value <= 1 —
    at most 28 blends behind the last opaque one, the premultiply, the average."""
    expect, translucent = M.image(stacks, msaa, bits, shifts)
    assert translucent <= 28
    if all(st.color == (1.0, 1.0, 1.0, 1.0) for st in stacks):
        return expect, 0.0
    return expect, 0.5 / 255.0 + 32 * 2.0 ** -24


def check_image(image, expect, tol, msaa, what):
    assert image.shape == (M.SIZE, M.SIZE, 4) and image.dtype == np.uint8
    if tol == 0.0:  # white or nothing per sample: k covered samples of msaa resolve to round(255 k / msaa)
        got = np.rint(image.astype(np.float64) / 255.0 * msaa)
        want = np.rint(expect * msaa)
        bad = (got != want).any(axis=2) | (np.abs(image.astype(np.float64) / 255.0 - expect) > 0.5 / 255.0 + 2.0 ** -20).any(axis=2)
    else:
        bad = (np.abs(image.astype(np.float64) / 255.0 - expect) > tol).any(axis=2)
    assert not bad.any(), f"{what}: {int(bad.sum())} pixels differ from the count model, first (y, x) {np.argwhere(bad)[:4].tolist()}: got {image[bad][:4].tolist()}, model {np.round(expect[bad][:4] * 255, 3).tolist()}"


def counters_of(frame):
    out = (C.c_uint32 * 8)()
    frame.lib.crh_debug_frame_counters(frame.handle, out)
    return list(out)


def last_pass(frame):
    from test_gpu_fuzz import last_pass as tap
    return tap(frame)


@pytest.fixture
def no_pins(monkeypatch):
    import torch
    assert torch.cuda.is_available()
    from test_gpu_fuzz import _no_path_pins
    _no_path_pins(monkeypatch)


class Device:
    """One Renderer, Scene and Frame under one pin."""

    def __init__(self, monkeypatch, path, stacks, msaa, bits, batch=None):
        from contrast_renderer_amd import renderer as R
        for name, value in GPU_PATHS[path]:
            monkeypatch.setenv(name, value)
        self.path, self.msaa, self.stacks = path, msaa, stacks
        self.r = R.Renderer(R.Configuration(msaa_sample_count=msaa, clip_nesting_counter_bits=0, winding_counter_bits=bits), device=0)
        self.scene = R.Scene(self.r, batch if batch is not None else batch_of(stacks))
        assert self.scene.status() == 0
        self.frame = R.Frame(self.r, M.SIZE, M.SIZE)
        self.colors = np.float32([st.color for st in stacks])

    def draw(self, shifts=None, scene=None, transforms=None, colors=None):
        """One pass into the cleared frame -> (image, last_pass, counters)."""
        if transforms is None:
            transforms = np.stack([M.transform(st.shift if shifts is None else shifts[k]) for k, st in enumerate(self.stacks)])
        self.frame.clear()
        (scene or self.scene).render(self.frame, transforms, self.colors if colors is None else colors)
        image = self.frame.download()
        return image, last_pass(self.frame), counters_of(self.frame)


def longest_expected(path, family, n):
    """The longest list the pass of `path` reports for a scene built for n entries of the edge formulation. The triangle pass bins strip
    triangles, not edges — other lists, longer ones: the two fill triangles of every rectangle and the two of every Shape's cover."""
    if path != "triangles":
        return n
    if family == "many":
        return 4 * (n // MANY_PER_SHAPE) + 4 * (n % MANY_PER_SHAPE)
    return 2 * (n - DEEP_EXTRA) + 2


def packed_kernel_expected(path, msaa):
    return msaa == 1 and path in ("default", "rows")


def assert_regime(path, family, n, msaa, k, t, counters, gated):
    """The kernel of pass k (0: verified, later: lists in place) and its longest list."""
    what = (family, n, msaa, path, k, t, counters)
    if gated and path in ("default", "rows"):
        # at and above the gate the frame leaves the packed kernels: the per-sample edge kernel draws it, under either pin
        assert t["general"] == 0 and t["raster"] in ("edges", "edges-long"), what
    else:
        assert path_ran(path, msaa, True, t), what
    want = longest_expected(path, family, n)
    # (a pass with its lists in place reports lists beyond the LDS sort only, raster_tile_list.hpp tile_list_range; a verified pass all)
    reported = k == 0 or n > LDS_SORT_MAX[msaa]
    if reported or path == "triangles":  # (the triangle pass measures every pass)
        assert counters[3] == want, what
    assert counters[0] == 0 and counters[5] == 0 and counters[2] == 0, what


# ---------------------------------------------------------------- the sizes, every raster path

SIZES = [1000, LDS_SORT_MAX[1], LDS_SORT_MAX[1] + 1, GATE - 1, GATE, IN_PLACE_MAX, 2 * GATE + 232]  # the last: beyond 2^15, the kernels that stay in use there
FAMILIES = ["deep-cw", "deep-reversed", "deep-mixed", "many"]
PATHS = {1: ["default", "rows", "edges", "triangles"], 4: ["edges", "triangles"]}


CASES = [(f, n, b) for f in FAMILIES for n in SIZES for b in (1, 4, 8) if b == 8 or f == "many" or n != SIZES[-1]]  # (the largest single Shape: the 8-bit case only)


@pytest.mark.gpu
@pytest.mark.parametrize("family,n,bits", CASES, ids=[f"{f}-{n}-bits{b}" for f, n, b in CASES])
def test_every_path_draws_the_count_model(family, n, bits, no_pins, monkeypatch):
    """Each size at winding_counter_bits 1, 4, 8; msaa 1 on fill, rows, edges, triangles and msaa 4 on edges, triangles; the verified pass
    and the pass with the lists in place. All paths are exact for the deep family, so their bytes are equal as well."""
    gated = n >= GATE
    if True:
        stacks, batch = scene_of(family, n, bits)
        if family == "deep-mixed":  # the case is what it says: covered samples, and uncovered ones whose count is a multiple of 2^bits but not 0
            cnt = M.counts(stacks[0], 1)
            assert ((cnt != 0) & (cnt % (1 << bits) == 0)).any() and (cnt % (1 << bits) != 0).any() and (cnt < 0).any() and (cnt > 0).any(), (n, bits)
        for msaa in (1, 4):
            expect, tol = expected_bytes(stacks, msaa, bits)
            assert 0.0 < (expect[..., 3] > 0).mean() < 1.0  # (something is drawn, and not everywhere)
            first = None
            for path in PATHS[msaa]:
                d = Device(monkeypatch, path, stacks, msaa, bits, batch)
                for k in range(2):
                    image, t, counters = d.draw()
                    assert_regime(path, family, n, msaa, k, t, counters, gated)
                    assert k == 0 or t["direct"] or path == "triangles", (family, n, path, t)
                    if not gated and packed_kernel_expected(path, msaa):
                        assert t["raster"] in ("fill", "rows", "rows-long"), (family, n, path, t)
                    check_image(image, expect, tol, msaa, f"{family} n={n} bits={bits} msaa={msaa} {path} pass {k} {t} {counters}")
                    if tol == 0.0:
                        first = image if first is None else first
                        assert np.array_equal(image, first), (family, n, bits, msaa, path, k)
                _no_pins_again(monkeypatch)


def _no_pins_again(monkeypatch):
    from test_gpu_fuzz import _no_path_pins
    _no_path_pins(monkeypatch)


# ---------------------------------------------------------------- the gate

@pytest.mark.gpu
@pytest.mark.parametrize("path", ["default", "rows"])
@pytest.mark.parametrize("family", ["deep-mixed", "many"])
def test_the_gate_takes_the_frame_off_the_packed_kernels_and_is_sticky(family, path, no_pins, monkeypatch):
    """A list of GATE entries: the verified pass measures it before its raster kernel runs, and no pass of that frame — that one included —
    runs fill, rows or rows-long. The gate is `has ever shown` (crh_frame::longest_list is a maximum over the frame's passes): a small
    scene drawn into the same frame afterwards stays on the per-sample kernel, while the same small scene in a fresh frame takes the packed one."""
    bits = 8
    stacks = stacks_of(family, GATE, bits)
    expect, tol = expected_bytes(stacks, 1, bits)
    d = Device(monkeypatch, path, stacks, 1, bits)
    for k in range(3):
        image, t, counters = d.draw()
        assert t["raster"] in ("edges", "edges-long"), (k, t, counters)
        assert counters[3] == GATE, (k, t, counters)
        check_image(image, expect, tol, 1, f"gate {family} {path} pass {k} {t} {counters}")
    from contrast_renderer_amd import renderer as R
    small = stacks_of(family, 1000, bits)
    small_scene = R.Scene(d.r, batch_of(small))
    small_t = np.stack([M.transform(st.shift) for st in small])
    small_c = np.float32([st.color for st in small])
    small_expect, small_tol = expected_bytes(small, 1, bits)
    for k in range(3):
        image, t, counters = d.draw(scene=small_scene, transforms=small_t, colors=small_c)
        assert t["raster"] in ("edges", "edges-long"), ("sticky", k, t, counters)
        check_image(image, small_expect, small_tol, 1, f"gate, small scene afterwards, {family} {path} pass {k} {t} {counters}")
    fresh = R.Frame(d.r, M.SIZE, M.SIZE)
    fresh.clear()
    small_scene.render(fresh, small_t, small_c)
    image = fresh.download()
    assert path_ran(path, 1, True, last_pass(fresh)), last_pass(fresh)
    check_image(image, small_expect, small_tol, 1, "the small scene in a fresh frame")


# ---------------------------------------------------------------- growth between two verified passes

def growth_stacks(family):
    """Three groups A, B, C on one tile column: A alone makes GATE - 1 entries, A + B IN_PLACE_MAX - 1 (inside A's places), A + B + C more
    than the places B's pass leaves. B and C wait 64 pixels to the right of the frame until their pass slides them in."""
    a, b = GATE - 1, IN_PLACE_MAX - 1 - (GATE - 1)
    c = place_capacity(IN_PLACE_MAX - 1) - (IN_PLACE_MAX - 1) + 90
    if family == "many":
        groups = [many_stacks(a), many_stacks(b - b % MANY_PER_SHAPE), many_stacks(c - c % MANY_PER_SHAPE)]
        sizes = [a, b - b % MANY_PER_SHAPE, c - c % MANY_PER_SHAPE]
    else:
        # (one Shape each: the first deeply positive then negative, the second reversed, the third clockwise; its own DEEP_EXTRA entries each)
        groups = [deep_stack("mixed", a), deep_stack("reversed", b), deep_stack("cw", c)]
        for g, color in zip(groups, [(1.0, 1.0, 1.0, 1.0), (0.25, 0.5, 1.0, 1.0), (1.0, 0.5, 0.125, 0.5)]):
            g[0].color = color
        sizes = [a, b, c]
    return groups, sizes


@pytest.mark.gpu
@pytest.mark.parametrize("path", ["default", "rows"])
@pytest.mark.parametrize("family", ["deep", "many"])
def test_growth_between_verified_passes(family, path, no_pins, monkeypatch):
    """One Scene, one Frame, lists in place. Pass A (twice: verified, then in place) shows GATE - 1 entries on the packed kernel; pass B
    slides a second group onto the same tiles — the lists grow to IN_PLACE_MAX - 1 entries, the capacity of their places, with nothing
    measured in between —; pass C outgrows the places B's pass leaves (the pass draws nothing, is noticed and drawn again the verified way,
    above the gate). Every image is the count model's, and each assertion's message says which kernel drew which pass, in place or verified."""
    bits = 8
    groups, sizes = growth_stacks(family)
    stacks = [st for g in groups for st in g]
    group_of = np.concatenate([np.full(len(g), i) for i, g in enumerate(groups)])
    away = 64.0
    d = Device(monkeypatch, path, stacks, 1, bits)
    packed = ("fill",) if path == "default" else ("rows", "rows-long")
    log = []

    def run(name, present, want_longest):
        shifts = [st.shift if present[group_of[k]] else st.shift + away for k, st in enumerate(stacks)]
        expect, tol = expected_bytes(stacks, 1, bits, shifts)
        image, t, counters = d.draw(shifts)
        log.append((name, t["raster"], "in place" if t["direct"] else "verified", counters[:8]))
        check_image(image, expect, tol, 1, f"growth {family} {path}: {log}")
        assert counters[3] == want_longest, log
        return t

    t = run("A", (True, False, False), sizes[0])
    assert t["raster"] in packed and not t["direct"], log
    t = run("A again", (True, False, False), sizes[0])
    assert t["raster"] in packed and t["direct"], log
    assert GATE <= sizes[0] + sizes[1] <= IN_PLACE_MAX
    t = run("B", (True, True, False), sizes[0] + sizes[1])
    # Either the lists fitted the places pass A left and the packed kernel drew them in place (exact: below 2^15 entries), or the pass was
    # noticed and drawn again the verified way, which is above the gate and so on the per-sample kernel. Nothing else is right — a packed
    # kernel behind a verified pass would mean the gate did not hold. (Observed: the second, `edges-long`, verified, for all four cases.)
    assert (t["raster"] in packed and t["direct"]) or (t["raster"] in ("edges", "edges-long") and not t["direct"]), log
    assert sum(sizes) > place_capacity(sizes[0] + sizes[1])
    t = run("C", (True, True, True), sum(sizes))
    assert t["raster"] in ("edges", "edges-long") and not t["direct"], log  # outgrown: drawn again the verified way, above the gate
    t = run("C again", (True, True, True), sum(sizes))
    assert t["raster"] in ("edges", "edges-long"), log


# ---------------------------------------------------------------- the model against the oracle, on the CPU

@pytest.mark.parametrize("family", FAMILIES)
def test_the_count_model_equals_the_oracle(family, oracle_lib):
    """n = 600, msaa 1 and 4, bits 1, 4, 8: byte for byte for the opaque deep stacks, within the RGBA8 tolerance for `many`."""
    from oracle.binding import Oracle
    n = 600
    for bits in (1, 4, 8):
        stacks = stacks_of(family, n, bits)
        o = Oracle(batch_of(stacks))
        assert o.status() == 0
        transforms = np.stack([M.transform(st.shift) for st in stacks])
        colors = np.float32([st.color for st in stacks])
        for msaa in (1, 4):
            expect, tol = expected_bytes(stacks, msaa, bits)
            image = o.render(M.SIZE, M.SIZE, msaa, bits, transforms, colors)
            check_image(image, expect, tol, msaa, f"oracle {family} bits={bits} msaa={msaa}")
            if tol == 0.0:
                exact = np.floor(expect * 255.0 + 0.5).astype(np.uint8)
                assert np.array_equal(image[..., 3] == 0, exact[..., 3] == 0) and (msaa != 1 or np.array_equal(image, exact))
