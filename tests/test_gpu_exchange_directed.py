"""Directed tests of the multi-GPU exchange (csrc/comm.hip) over loopback groups on one device, against the exact host model of
tests/exchange_model.py: layers of chosen bytes (Frame.upload) or, for RGBA16F, of pixel-aligned rectangles drawn one Shape each, so that
which tiles are occupied, which bitmap words and slabs they fall in and what the composite has to do to them is under the test's control.
Every exchange is checked three ways: the result equals the model byte for byte, the pixels of tiles no layer occupies are zero, and — where
the occupancy comes from scanning the pixels — crh_comm_last_peer_bytes and crh_comm_last_traffic of every rank equal the model's figures."""
import numpy as np
import pytest

from contrast_renderer_amd import renderer as R

import exchange_model as M
from exchange_util import assert_traffic, rect_scene

pytestmark = pytest.mark.gpu
ERR_UNSUPPORTED, ERR_INVALID_ARGUMENT = 8, 10


class Device:
    """One renderer per sample count and one loopback group per world size, shared by the tests of the module: the groups are reused across sizes and formats."""

    def __init__(self):
        import torch
        assert torch.cuda.is_available()
        self.renderers, self.groups = {}, {}

    def renderer(self, msaa=1):
        if msaa not in self.renderers:
            self.renderers[msaa] = R.Renderer(R.Configuration(msaa, 4, 4), device=0)
        return self.renderers[msaa]

    def group(self, world, msaa=1):
        if (world, msaa) not in self.groups:
            r = self.renderer(msaa)
            comms = [R.Comm(r, 0, world)]
            comms += [R.Comm(r, k, world, rank0=comms[0]) for k in range(1, world)]
            self.groups[(world, msaa)] = comms
        return self.groups[(world, msaa)]


@pytest.fixture(scope="module")
def device():
    return Device()


def uploaded(r, layers):
    frames = []
    for pixels in layers:
        h, w = pixels.shape[:2]
        frame = R.Frame(r, w, h)
        frame.upload(pixels)
        frames.append(frame)
    return frames


def assert_image(image, layers, where=""):
    """The three properties of a result, the traffic apart: `layers` = what the layers held ([world, h, w, 4])."""
    layers = np.asarray(layers)
    expect = M.composite(layers)
    bad = (image != expect).any(axis=2)
    assert not bad.any(), f"{where}: {int(bad.sum())} of {bad.size} pixels differ from the model, first at (row, column) {tuple(int(v) for v in np.argwhere(bad)[0])}"
    union = np.stack([M.occupancy(layer) for layer in layers]).any(axis=0)
    assert not image[~M.tile_pixels(union, image.shape[1], image.shape[0])].any(), f"{where}: a tile no layer occupies is not transparent"


def exchange_and_check(comms, frames, result, layers, where="", scanned=True):
    comms[0].local_exchange(frames, result)
    image = result.download()
    assert_image(image, layers, where)
    if scanned:
        assert_traffic(comms, M.traffic_of_layers(np.asarray(layers)), where)
    return image


def solid(rng, width, height, mask, opaque_share=0.2):
    """Random premultiplied bytes with alpha >= 1 on the pixels of `mask`, zero elsewhere: every tile the mask touches is occupied."""
    pixels = M.random_premultiplied(rng, width, height, opaque_share)
    pixels[..., 3] = np.maximum(pixels[..., 3], 1)
    return pixels * mask[..., None].astype(np.uint8)


# ---------------------------------------------------------------------------------------------- geometry: one byte, one tile

@pytest.mark.parametrize("size", [(1, 1), (16, 16), (17, 17), (15, 33), (129, 47), (132, 40), (500, 16), (528, 16)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_a_single_non_zero_byte_moves_exactly_one_tile(size, device):
    """One non-zero byte in otherwise empty layers — at every corner of the frame, at the last pixel of the first tile, at the first pixel of the
    last (partial) tile and at the end of the first tile row —, in each of the four channels in turn (a colour byte under alpha 0 is content):
    exactly that tile travels, from the rank that holds it to the owner of its slab and from there to rank 0. Widths that are no multiple of
    4 take the scalar branch of the frame loads and stores; 528 / 16 = 33 tiles put a bitmap word's end inside the tile row."""
    w, h = size
    world = 2 if w * h <= 17 * 17 else 3
    r, comms = device.renderer(), device.group(world)
    tx, ty = M.tile_grid(w, h)
    places = sorted({(0, 0), (w - 1, 0), (0, h - 1), (w - 1, h - 1), (min(15, w - 1), min(15, h - 1)), ((tx - 1) * 16, (ty - 1) * 16), (w - 1, min(15, h - 1)), (min(w - 1, 31 * 16 + 15), 0)})
    frames = [R.Frame(r, w, h) for _ in range(world)]
    result = R.Frame(r, w, h)
    step = 0
    for x, y in places:
        for channel in range(4):
            rank = step % world
            layers = np.zeros((world, h, w, 4), dtype=np.uint8)
            layers[rank, y, x, channel] = (1, 255, 128)[step % 3]
            for f, pixels in zip(frames, layers):
                f.upload(pixels)
            where = f"{w}x{h}, byte {int(layers[rank, y, x, channel])} at pixel ({x}, {y}) channel {channel} of rank {rank}'s layer"
            image = exchange_and_check(comms, frames, result, layers, where)
            tile = (y // 16) * tx + x // 16
            occupied = np.stack([M.occupancy(layer) for layer in layers])
            assert occupied.sum() == 1 and occupied[rank, tile], where
            owner = [k for k in range(world) if M.slab_tiles(tx, ty, k, world)[0] <= tile < M.slab_tiles(tx, ty, k, world)[1]][0]
            assert sum(c.last_traffic()[0] for c in comms) == 1024 * (int(owner != rank) + int(owner != 0)), where  # one tile: to its slab's owner, and on to rank 0
            assert image.any(), where
            step += 1


# ---------------------------------------------------------------------------------------------- bitmap words and slabs

PATTERNS = ("all", 0, 31, 32, 33, 63, 64, "last", "checker", "every 32nd", "every 32nd from 31", "none")


def pattern(which, tiles_x, tiles_y):
    n = tiles_x * tiles_y
    t = np.arange(n)
    if which == "all":
        return np.ones(n, dtype=bool)
    if which == "none":
        return np.zeros(n, dtype=bool)
    if which == "checker":
        return (t // tiles_x + t % tiles_x) % 2 == 0
    if which == "every 32nd":
        return t % 32 == 0
    if which == "every 32nd from 31":
        return t % 32 == 31
    return t == (n - 1 if which == "last" else which)


@pytest.mark.parametrize("world", [3, 5, 7])
@pytest.mark.parametrize("size", [(141, 125), (200, 91)], ids=["9x8 tiles", "13x6 tiles"])
def test_tile_patterns_across_bitmap_words_and_slabs(size, world, device):
    """72 and 78 tiles are three bitmap words, and a row of 9 or 13 tiles puts every slab's first tile in the middle of a word (tile_rank,
    host_rank, segment). Twelve patterns — every tile, one tile on either side of a word's end, a checkerboard, every 32nd tile, none — turn
    through the ranks, so that every rank's layer has another pattern in every exchange and the union is none of them."""
    w, h = size
    tx, ty = M.tile_grid(w, h)
    assert tx in (9, 13) and tx * ty > 65
    r, comms = device.renderer(), device.group(world)
    rng = np.random.RandomState(w + world)
    frames = [R.Frame(r, w, h) for _ in range(world)]
    result = R.Frame(r, w, h)
    for e in range(len(PATTERNS)):
        names = [PATTERNS[(e + k) % len(PATTERNS)] for k in range(world)]
        layers = np.stack([solid(rng, w, h, M.tile_pixels(pattern(name, tx, ty), w, h)) for name in names])
        occupied = np.stack([M.occupancy(layer) for layer in layers])
        assert all(np.array_equal(occupied[k], pattern(names[k], tx, ty)) for k in range(world))
        assert not any(np.array_equal(occupied.any(axis=0), occupied[k]) for k in range(world)) or "all" in names
        for f, pixels in zip(frames, layers):
            f.upload(pixels)
        exchange_and_check(comms, frames, result, layers, f"{w}x{h}, world {world}, patterns {names}")


def test_rgba16f_layers_of_drawn_rectangles(device, monkeypatch):
    """RGBA16F layers cannot be uploaded: they are drawn, one Shape per pixel-aligned rectangle, and downloaded for the model. A 16F target
    stores the resolved colour clamped to [0, 1] (store_pixel), so no half is above 1. Rectangles inside tiles 0, 31, 32, 33, 63, 64 and the
    last one, a single pixel in the corner of the partial last column (141 is no multiple of 4: the scalar loads), an opaque rectangle over
    several tiles and translucent ones above it; the occupancy is scanned (CRH_EXCHANGE_SCAN_PIXELS), so the traffic — 2 KiB layer tiles, 1
    KiB composited ones — is the model's exactly."""
    monkeypatch.setenv("CRH_EXCHANGE_SCAN_PIXELS", "1")
    w, h, world = 141, 125, 3
    tx, ty = M.tile_grid(w, h)
    r, comms = device.renderer(), device.group(world)

    def inside(tile, margin=3):
        x0, y0, x1, y1 = M.tile_rect(tile, w, h)
        return (x0 + margin, y0 + margin, x1 - 1, y1 - 1) if x1 - x0 > margin + 1 and y1 - y0 > margin + 1 else (x0, y0, x1, y1)

    last = tx * ty - 1
    plans = [
        ([inside(0), inside(32), inside(63), (20, 96, 100, 110)], [(1.0, 0.5, 0.25, 1.0), (0.2, 0.4, 0.6, 0.5), (0.0, 1.0, 0.0, 0.25), (0.9, 0.1, 0.3, 1.0)]),
        ([inside(31), inside(33), inside(64), (140, 0, 141, 1), (60, 70, 120, 110)], [(0.3, 0.3, 0.3, 0.3), (1.0, 1.0, 1.0, 1.0), (0.5, 0.0, 0.5, 0.75), (0.0, 0.0, 1.0, 1.0), (0.1, 0.8, 0.2, 0.4)]),
        ([inside(last), inside(32, 5), (140, 124, 141, 125), (0, 100, 50, 125)], [(0.7, 0.2, 0.1, 0.6), (0.0, 0.0, 0.0, 0.5), (1.0, 0.0, 0.0, 0.5), (0.6, 0.6, 0.0, 0.9)]),
    ]
    frames, keep = [], []
    for rects, colors in plans:
        scene, t = rect_scene(r, w, h, rects)
        frame = R.Frame(r, w, h, R.FORMAT_RGBA16F)
        frame.clear()
        scene.render(frame, t, np.float32(colors))
        frames.append(frame)
        keep.append(scene)
    halves = np.stack([f.download() for f in frames])
    assert halves.dtype == np.float16 and halves.max() <= 1.0 and halves.min() >= 0.0
    occupied = np.stack([M.occupancy(layer) for layer in halves])
    for tile, rank in ((0, 0), (32, 0), (63, 0), (31, 1), (33, 1), (64, 1), (8, 1), (last, 2), (32, 2)):
        assert occupied[rank, tile], (tile, rank)  # the rectangles are where they were meant to be
    assert not occupied[0, 31] and not occupied[1, 32] and not occupied[2, 0] and M.pixel_nonzero(halves[1])[0, 140] and M.pixel_nonzero(halves[2])[124, 140]
    result = R.Frame(r, w, h)
    image = exchange_and_check(comms, frames, result, halves, "three drawn RGBA16F layers")
    assert image.any()
    swapped = exchange_and_check(comms, [frames[1], frames[0], frames[2]], result, halves[[1, 0, 2]], "the same layers, the lower two swapped")
    assert not np.array_equal(image, swapped)
    # the same group goes back to RGBA8 layers of the same size: 1 KiB tiles again
    bytes8 = np.stack([solid(np.random.RandomState(k), w, h, M.tile_pixels(occupied[k], w, h)) for k in range(world)])
    exchange_and_check(comms, uploaded(r, bytes8), result, bytes8, "RGBA8 layers after RGBA16F ones")


# ---------------------------------------------------------------------------------------------- world sizes

def world_layers(world, w, h, seed):
    """Layers whose order shows: tile 0 has every layer, translucent; tile 1 only the last layer; tile 2 only layer 8 and tile 3 only layer 16
    (where they exist); tile 4 nothing; tile 5 an opaque layer 0 under translucent others; the rest a random subset of ranks each, a fifth of
    the pixels opaque."""
    rng = np.random.RandomState(seed)
    tx, ty = M.tile_grid(w, h)
    n = tx * ty
    has = rng.uniform(size=(world, n)) < 0.5
    has[:, 0] = True
    has[:, 1:5] = False
    has[world - 1, 1] = True
    if world > 8:
        has[8, 2] = True
    if world > 16:
        has[16, 3] = True
    has[:, 5] = True
    layers = np.stack([solid(rng, w, h, M.tile_pixels(has[k], w, h)) for k in range(world)])
    x0, y0, x1, y1 = M.tile_rect(0, w, h)
    layers[:, y0:y1, x0:x1, 3] = np.minimum(layers[:, y0:y1, x0:x1, 3], 200)  # tile 0: nobody hides what is underneath
    layers[:, y0:y1, x0:x1, :3] = np.minimum(layers[:, y0:y1, x0:x1, :3], layers[:, y0:y1, x0:x1, 3:4])
    x0, y0, x1, y1 = M.tile_rect(5, w, h)
    layers[0, y0:y1, x0:x1] = (200, 100, 50, 255)
    return layers, has


@pytest.mark.parametrize("world,size", [(1, (64, 64)), (2, (64, 64)), (8, (64, 64)), (9, (64, 64)), (16, (64, 64)), (17, (64, 64)), (9, (50, 40)), (17, (50, 40))],
                         ids=lambda v: str(v) if isinstance(v, int) else f"{v[0]}x{v[1]}")
def test_world_sizes_up_to_seventeen_keep_the_layer_order(world, size, device):
    """Four (or three) tile rows for up to seventeen ranks: most slabs are empty, the composite loads its layers in batches of eight, and a tile
    only the ninth or the seventeenth layer has must arrive. "Over" does not commute: the layers swapped give other bytes, by the model and
    by the exchange."""
    w, h = size
    r, comms = device.renderer(), device.group(world)
    layers, has = world_layers(world, w, h, 100 * world + w)
    tx, ty = M.tile_grid(w, h)
    assert sum(1 for k in range(world) if M.slab_tiles(tx, ty, k, world)[0] == M.slab_tiles(tx, ty, k, world)[1]) == max(0, world - ty)
    frames = uploaded(r, layers)
    result = R.Frame(r, w, h)
    image = exchange_and_check(comms, frames, result, layers, f"world {world}")
    for tile, rank in ((1, world - 1), (2, 8), (3, 16)):
        if rank < world:
            x0, y0, x1, y1 = M.tile_rect(tile, w, h)
            assert np.array_equal(image[y0:y1, x0:x1], layers[rank, y0:y1, x0:x1]), (tile, rank)  # alone in its tile: the layer's own bytes
    if world > 1:
        for a, b in {(0, world - 1), (0, 1), (world - 2, world - 1), (min(7, world - 2), min(8, world - 1))}:
            order = list(range(world))
            order[a], order[b] = order[b], order[a]
            assert not np.array_equal(M.composite(layers[order]), M.composite(layers)), (a, b)
            swapped = exchange_and_check(comms, [frames[k] for k in order], result, layers[order], f"world {world}, layers {a} and {b} swapped")
            assert not np.array_equal(swapped, image)
    # every rank's layer all 255: the accumulator is 1 + 0 * 0 at every step
    white = np.full((world, h, w, 4), 255, dtype=np.uint8)
    image = exchange_and_check(comms, uploaded(r, white), result, white, f"world {world}, all 255")
    assert (image == 255).all()


# ---------------------------------------------------------------------------------------------- long bitmaps

@pytest.mark.parametrize("height", [58240, 58256])
def test_bitmaps_of_1024_and_1025_words(height, device):
    """129 x 58240 is 9 x 3640 = 32760 tiles = 1024 bitmap words, one word per thread of k_bit_prefix; sixteen more rows give 32769 tiles =
    1025 words, two words per thread. Occupied: tile 0, the tiles around index 32768, the last tile and about 1 % at random, other tiles in
    each of the two layers. The host composites the tile rows that hold anything and asserts that the rest of the 30 MB image is zero."""
    w, world = 129, 2
    tx, ty = M.tile_grid(w, height)
    n = tx * ty
    assert M.n_words(w, height) == (1024 if height == 58240 else 1025)
    r, comms = device.renderer(), device.group(world)
    rng = np.random.RandomState(height)
    around = [t for t in range(32700, 32800) if t < n]
    chosen = [sorted(set([0] + around[0::2] + [int(v) for v in rng.randint(0, n, n // 100)])),
              sorted(set([n - 1, 16379, 16380] + around[1::3] + [int(v) for v in rng.randint(0, n, n // 100)]))]
    layers = np.zeros((world, height, w, 4), dtype=np.uint8)
    for k in range(world):
        for tile in chosen[k]:
            x0, y0, x1, y1 = M.tile_rect(tile, w, height)
            block = M.random_premultiplied(rng, x1 - x0, y1 - y0)
            block[..., 3] = np.maximum(block[..., 3], 1)
            layers[k, y0:y1, x0:x1] = block
    occupied = np.stack([M.occupancy(layer) for layer in layers])
    assert all(sorted(np.flatnonzero(occupied[k])) == chosen[k] for k in range(world)) and occupied[1, n - 1] and occupied[0, 0]
    frames = uploaded(r, layers)
    result = R.Frame(r, w, height)
    comms[0].local_exchange(frames, result)
    image = result.download()
    union = occupied.any(axis=0)
    rows = np.repeat(union.reshape(ty, tx).any(axis=1), 16)[:height]
    assert np.array_equal(image[rows], M.composite(layers[:, rows])), f"height {height}: the occupied tile rows differ from the model"
    assert not image[~rows].any() and not image[~M.tile_pixels(union, w, height)].any()
    assert_traffic(comms, M.traffic(occupied, w, height), f"height {height}")


# ---------------------------------------------------------------------------------------------- arithmetic

def test_every_backdrop_source_and_alpha_byte_through_the_composite(device):
    """Two layers in which every (backdrop byte, source byte, source alpha) triple occurs in a colour channel — 256^3 channel values, three to
    a pixel, 5.6 million pixels — and every (backdrop alpha, source alpha) pair in alpha. The bottom layer passes through the first step
    unchanged (b + 0 * keep), so the second step computes s + b * (1 - a) for every triple: with one rounding per operation (no fused
    multiply-add: -ffp-contract=off) and the quantisation's + 0.5 the bytes are the model's."""
    per_alpha = (65536 + 2) // 3  # pixels that hold the 65536 (backdrop, source) pairs of one source alpha
    w, h, world = 2048, (256 * per_alpha + 2047) // 2048, 2
    pairs = np.zeros(per_alpha * 3, dtype=np.int64)
    pairs[:65536] = np.arange(65536)
    pairs = pairs.reshape(per_alpha, 3)
    back = np.zeros((256, per_alpha, 4), dtype=np.uint8)
    src = np.zeros((256, per_alpha, 4), dtype=np.uint8)
    back[..., :3], src[..., :3] = pairs >> 8, pairs & 255
    src[..., 3] = np.arange(256)[:, None]
    back[..., 3] = np.arange(per_alpha)[None, :] % 256
    layers = np.zeros((world, h * w, 4), dtype=np.uint8)
    layers[0, :256 * per_alpha], layers[1, :256 * per_alpha] = back.reshape(-1, 4), src.reshape(-1, 4)
    layers = layers.reshape(world, h, w, 4)
    seen = np.zeros(1 << 24, dtype=bool)
    for c in range(3):
        seen[(layers[0, ..., c].astype(np.int64) << 16 | layers[1, ..., c].astype(np.int64) << 8 | layers[1, ..., 3]).reshape(-1)] = True
    assert seen.all()
    assert len(np.unique(layers[0, ..., 3].astype(np.int64) << 8 | layers[1, ..., 3])) == 65536
    r, comms = device.renderer(), device.group(world)
    exchange_and_check(comms, uploaded(r, layers), R.Frame(r, w, h), layers, "every byte triple")


@pytest.mark.parametrize("world", [3, 9])
def test_layers_that_are_not_premultiplied_reach_the_clamp(world, device):
    """Random bytes, colour above alpha more often than not: the accumulator leaves [0, 1] and the quantisation clamps it."""
    w, h = 100, 70
    rng = np.random.RandomState(world)
    layers = rng.randint(0, 256, (world, h, w, 4)).astype(np.uint8)
    layers[:, :, :30, 3] = rng.randint(0, 40, (world, h, 30))  # nearly transparent sources that add their colour: sums far above 1
    acc = np.zeros((h, w, 4))
    for layer in layers:
        s = layer / 255.0
        acc = s + acc * (1.0 - s[..., 3:4])
    assert (acc[..., :3] > 1.0).mean() > 0.1 and (acc <= 1.0).any()
    r, comms = device.renderer(), device.group(world)
    image = exchange_and_check(comms, uploaded(r, layers), R.Frame(r, w, h), layers, f"{world} random layers")
    assert (image[acc > 1.0 + 1e-4] == 255).all()


# ---------------------------------------------------------------------------------------------- the two sources of the occupancy

@pytest.mark.parametrize("msaa", [1, 4])
def test_occupancy_from_tile_counts_against_the_pixel_scan(msaa, device, monkeypatch):
    """Rendered layers, exchanged once as the code chooses — the occupancy from the tile counts of the layer's pass where they describe the
    pixels — and once with CRH_EXCHANGE_SCAN_PIXELS set (it is read on every call). 160 x 112 is 10 x 7 tiles; world 3 has the tile rows 0-2,
    3-4 and 5-6. Rank 0's layer holds a Shape drawn with colour (0, 0, 0, 0) over four tiles of rank 2's slab that nothing else touches: those
    tiles have entries and no pixels, so they travel when the counts are the source and do not when the pixels are. Rank 1's frame is
    restricted to its tile rows (set_tile_rows) under a scene that covers the frame. Rank 2's layer is drawn in two passes, the second one a
    LoadOp::Load pass whose counts say nothing about the first pass's tiles: it is scanned either way."""
    w, h, world = 160, 112, 3
    tx, ty = M.tile_grid(w, h)
    r, comms = device.renderer(msaa), device.group(world, msaa)
    clear = (16, 80, 48, 112)  # tiles (1..2, 5..6)
    scenes = [rect_scene(r, w, h, [(8.5, 4.5, 60.25, 40.0), (100, 50, 150, 100), clear]),
              rect_scene(r, w, h, [(0, 0, 160, 112), (30.25, 30.5, 90, 90)]),
              rect_scene(r, w, h, [(0, 0, 32, 32)]), rect_scene(r, w, h, [(120, 90, 160, 112), (70.5, 0, 75, 20)])]
    colors = [np.float32([(0.8, 0.3, 0.1, 0.6), (0.1, 0.2, 0.9, 1.0), (0.0, 0.0, 0.0, 0.0)]), np.float32([(0.2, 0.9, 0.4, 0.5), (1.0, 1.0, 0.0, 1.0)]),
              np.float32([(0.5, 0.5, 1.0, 1.0)]), np.float32([(0.9, 0.0, 0.9, 0.7), (0.0, 0.6, 0.6, 1.0)])]
    frames = [R.Frame(r, w, h) for _ in range(world)]
    frames[1].set_tile_rows(48, 80)
    for f in frames:
        f.clear()
    for k in range(3):
        scenes[k][0].render(frames[k], scenes[k][1], colors[k])
    scenes[3][0].render(frames[2], scenes[3][1], colors[3])  # the second pass of rank 2's layer: over its content
    result = R.Frame(r, w, h)
    monkeypatch.delenv("CRH_EXCHANGE_SCAN_PIXELS", raising=False)
    comms[0].local_exchange(frames, result)
    by_counts = result.download()
    counted = [(c.last_peer_bytes(), c.last_traffic()) for c in comms]
    monkeypatch.setenv("CRH_EXCHANGE_SCAN_PIXELS", "1")
    comms[0].local_exchange(frames, result)
    by_scan = result.download()
    scanned = [(c.last_peer_bytes(), c.last_traffic()) for c in comms]
    layers = np.stack([f.download() for f in frames])
    assert not layers[1, :48].any() and not layers[1, 80:].any() and layers[1, 48:80].all(axis=2).any()
    assert_image(by_scan, layers, f"msaa {msaa}, scanned")
    assert_image(by_counts, layers, f"msaa {msaa}, from the counts")
    assert np.array_equal(by_counts, by_scan)
    assert_traffic(comms, M.traffic_of_layers(layers), f"msaa {msaa}, scanned")
    for k in range(world):
        assert all(a >= b for a, b in zip(counted[k][0], scanned[k][0])) and counted[k][1][0] >= scanned[k][1][0] and counted[k][1][1] == scanned[k][1][1], (k, counted[k], scanned[k])
    occupied = M.occupancy(layers[0]).reshape(ty, tx)
    assert not occupied[5:7, 1:3].any() and not layers[0, 80:112, 16:48].any()  # the transparent Shape left no pixel ...
    assert counted[0][0][2] >= scanned[0][0][2] + 4 * 1024  # ... and its four tiles travelled to rank 2 when the counts were the source,
    assert scanned[0][0][2] == int(occupied[5:7].sum()) * 1024  # and did not when the pixels were
    assert counted[2][0] == scanned[2][0]  # a layer of two passes is scanned either way: what it sends its peers is the same
    assert counted[2][1][0] >= scanned[2][1][0] + 4 * 1024  # (what it returns to rank 0 holds the four tiles rank 0's counts named)
    first_pass = M.occupancy(layers[2]).reshape(ty, tx)
    assert first_pass[0:2, 0:2].all() and first_pass[6, 9] and scanned[2][0][0] >= 4 * 1024  # (the first pass's tiles are in rank 0's slab: they travel)


# ---------------------------------------------------------------------------------------------- errors, then recovery

def test_a_refused_exchange_leaves_the_group_usable(device):
    """A layer of another size, a layer of another format, a BGRA layer among RGBA8 ones (another format: InvalidArgument),
    BGRA layers throughout or a BGRA result (Unsupported: the composite is unorm RGBA), an RGBA16F result: each is an error of the call with its own status, and the next
    exchange of valid layers on the same group is exact, traffic included."""
    w, h, world = 64, 48, 2
    r, comms = device.renderer(), device.group(world)
    rng = np.random.RandomState(5)
    layers = np.stack([solid(rng, w, h, rng.uniform(size=(h, w)) < 0.02) for _ in range(world)])
    frames = uploaded(r, layers)
    result = R.Frame(r, w, h)
    exchange_and_check(comms, frames, result, layers, "before any error")
    small = R.Frame(r, 64, 32)
    small.upload(layers[1][:32])
    half = R.Frame(r, w, h, R.FORMAT_RGBA16F)
    bgra = R.Frame(r, w, h, R.FORMAT_BGRA8)
    bgra.upload(layers[1])
    bgra2 = R.Frame(r, w, h, R.FORMAT_BGRA8)
    bgra2.upload(layers[0])
    for name, bad_layers, bad_result, status in (("another size", [frames[0], small], result, ERR_INVALID_ARGUMENT), ("another size at rank 0", [small, frames[1]], result, ERR_INVALID_ARGUMENT),
                                                 ("another format", [frames[0], half], result, ERR_INVALID_ARGUMENT), ("a BGRA layer among RGBA8 ones", [frames[0], bgra], result, ERR_INVALID_ARGUMENT),
                                                 ("BGRA layers", [bgra, bgra2], result, ERR_UNSUPPORTED), ("a BGRA result", frames, bgra2, ERR_UNSUPPORTED),
                                                 ("an RGBA16F result", frames, half, ERR_INVALID_ARGUMENT)):
        with pytest.raises(R.ContrastError) as e:
            comms[0].local_exchange(bad_layers, bad_result)
        assert e.value.status == status, (name, e.value.status)  # refused for its own reason
        exchange_and_check(comms, frames[::-1], result, layers[::-1], f"after {name}")
        exchange_and_check(comms, frames, result, layers, f"after {name}, again")
    assert np.array_equal(bgra.download(), layers[1]) and np.array_equal(bgra2.download(), layers[0]) and np.array_equal(small.download(), layers[1][:32])  # the refused layers are what they were


# ---------------------------------------------------------------------------------------------- the result frame among the layers

def test_the_result_may_be_one_of_the_layers(device):
    """include/contrast_hip.h: `result` may be one of the layers, at any rank; the image is the composite of the layers as they were. Rank 0's
    communicator packs and unpacks on one stream; a layer of rank >= 1 is packed on that rank's stream, and rank 0's unpack is ordered behind
    every rank's packing, as every rank's packing is behind the unpack that wrote its layer. Three such exchanges back to back, each reading what the one before wrote, with no download in between."""
    w, h, world = 70, 50, 3
    r, comms = device.renderer(), device.group(world)
    rng = np.random.RandomState(11)
    a, b, c = [solid(rng, w, h, rng.uniform(size=(h, w)) < 0.3, 0.1) for _ in range(3)]
    fa, fb, fc = uploaded(r, [a, b, c])
    comms[0].local_exchange([fa, fb, fc], fa)  # the result is rank 0's layer
    a1 = M.composite(np.stack([a, b, c]))
    comms[0].local_exchange([fb, fa, fc], fc)  # ... rank 2's, and rank 1's layer is what the exchange before has just written
    c1 = M.composite(np.stack([b, a1, c]))
    comms[0].local_exchange([fa, fc, fb], fa)  # ... rank 0's again, over rank 1's layer, the result of the exchange before
    a2 = M.composite(np.stack([a1, c1, b]))
    assert_traffic(comms, M.traffic_of_layers(np.stack([a1, c1, b])), "the third exchange")
    assert np.array_equal(fa.download(), a2) and np.array_equal(fc.download(), c1) and np.array_equal(fb.download(), b)
    assert not np.array_equal(a2, a1) and not np.array_equal(c1, c)
