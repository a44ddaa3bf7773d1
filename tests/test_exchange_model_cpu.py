"""The host model of the exchange (tests/exchange_model.py) held stable without a GPU: its slabs against crh_comm_shard, its occupancy against a
plain loop over pixels, its traffic against a hand count, and its f32 composite against the same composite in float64."""
import numpy as np
import pytest

from contrast_renderer_amd import distributed as D

import exchange_model as M


def test_slabs_partition_the_tiles_for_every_grid_and_world():
    for tiles_y in range(1, 21):
        for world in range(1, 18):
            for tiles_x in (1, 9):
                at = 0
                for rank in range(world):
                    b, e = M.slab_tiles(tiles_x, tiles_y, rank, world)
                    assert b == at and e >= b and (e - b) % tiles_x == 0, (tiles_y, world, rank)
                    assert (b // tiles_x, e // tiles_x) == D.shard_range(tiles_y, rank, world)
                    at = e
                assert at == tiles_x * tiles_y
                rows = [M.slab_tiles(tiles_x, tiles_y, r, world) for r in range(world)]
                sizes = [(e - b) // tiles_x for b, e in rows]
                assert max(sizes) - min(sizes) <= 1 and sizes == sorted(sizes, reverse=True)  # the empty slabs are the last ranks'


def test_slabs_are_the_c_abis():
    from contrast_renderer_amd import renderer as R
    for tiles_y, world in ((1, 2), (4, 17), (9, 5), (20, 7), (3641, 2)):
        for rank in range(world):
            b, e = M.slab_tiles(13, tiles_y, rank, world)
            assert (b // 13, e // 13) == R.shard_range(tiles_y, rank, world)
            height = tiles_y * 16 - 5
            assert R.slab_rows(height, rank, world) == (min(height, b // 13 * 16), min(height, e // 13 * 16))


def _occupancy_by_loop(layer):
    h, w = layer.shape[:2]
    tx, ty = M.tile_grid(w, h)
    out = np.zeros(tx * ty, dtype=bool)
    for y in range(h):
        for x in range(w):
            for c in range(4):
                v = layer[y, x, c]
                if (int(np.uint16(np.float16(v).view(np.uint16)) & 0x7FFF) if layer.dtype == np.float16 else int(v)) != 0:
                    out[(y // 16) * tx + x // 16] = True
    return out


@pytest.mark.parametrize("size", [(1, 1), (16, 16), (17, 17), (15, 33), (37, 18)])
def test_occupancy_is_a_loop_over_the_pixels(size):
    w, h = size
    rng = np.random.RandomState(w * 100 + h)
    tx, ty = M.tile_grid(w, h)
    assert tx * ty == len(M.occupancy(np.zeros((h, w, 4), np.uint8)))
    for dtype in (np.uint8, np.float16):
        empty = np.zeros((h, w, 4), dtype=dtype)
        assert not M.occupancy(empty).any()
        if dtype == np.float16:
            empty[...] = np.float16(-0.0)  # the sign alone is no content
            assert empty.view(np.uint16).all() and not M.occupancy(empty).any()
        for _ in range(6):
            layer = np.zeros((h, w, 4), dtype=dtype)
            for _ in range(int(rng.randint(1, 4))):
                y, x, c = int(rng.randint(0, h)), int(rng.randint(0, w)), int(rng.randint(0, 4))
                layer[y, x, c] = 1 if dtype == np.uint8 else np.float16(rng.choice([6e-8, 1.0, -0.5]))  # (6e-8: the smallest subnormal half)
            got = M.occupancy(layer)
            assert np.array_equal(got, _occupancy_by_loop(layer)) and got.any()
            inside = M.tile_pixels(got, w, h)
            assert not M.pixel_nonzero(layer)[~inside].any() and inside.shape == (h, w)
    for t in range(tx * ty):
        x0, y0, x1, y1 = M.tile_rect(t, w, h)
        one = np.zeros(tx * ty, dtype=bool)
        one[t] = True
        mask = M.tile_pixels(one, w, h)
        assert mask[y0:y1, x0:x1].all() and mask.sum() == (y1 - y0) * (x1 - x0) > 0


def test_traffic_by_hand():
    """A 40 x 70 frame: 3 x 5 tiles; world 3 -> slabs of 2, 2 and 1 tile rows = tiles [0, 6), [6, 12), [12, 15)."""
    occ = np.zeros((3, 15), dtype=bool)
    occ[0, [0, 7, 8, 14]] = True   # rank 0: one tile at home, two for rank 1, one for rank 2
    occ[1, [1, 2, 6]] = True       # rank 1: two for rank 0, one at home
    occ[2, [7]] = True             # rank 2: one for rank 1 (a tile rank 0 has too)
    t = M.traffic(occ, 40, 70)
    assert [r["peer_bytes"] for r in t] == [[0, 2048, 1024], [2048, 0, 0], [0, 1024, 0]]
    # the union: tiles 0 1 2 | 6 7 8 | 14 -> rank 1 returns 3 composited tiles, rank 2 one, rank 0 none (it holds the result)
    assert [r["sent"] for r in t] == [3072, 2048 + 3 * 1024, 1024 + 1024]
    assert [r["dense"] for r in t] == [9 * 1024, 9 * 1024 + 6 * 1024, 12 * 1024 + 3 * 1024]
    half = M.traffic(occ, 40, 70, np.float16)  # 2 KiB layer tiles, 1 KiB composited ones
    assert [r["peer_bytes"] for r in half] == [[0, 4096, 2048], [4096, 0, 0], [0, 2048, 0]]
    assert [r["sent"] for r in half] == [6144, 4096 + 3 * 1024, 2048 + 1024]
    assert [r["dense"] for r in half] == [9 * 2048, 9 * 2048 + 6 * 1024, 12 * 2048 + 3 * 1024]
    # more ranks than tile rows: the last ranks have no slab, send their tiles and return nothing
    t = M.traffic(np.ones((7, 15), dtype=bool), 40, 70)
    assert [r["sent"] for r in t] == [12 * 1024] + [12 * 1024 + 3 * 1024] * 4 + [15 * 1024] * 2
    assert [r["dense"] for r in t][-1] == 15 * 1024 and t[6]["peer_bytes"] == [3072] * 5 + [0, 0]
    layers = np.zeros((2, 70, 40, 4), dtype=np.uint8)
    layers[1, 69, 39, 2] = 9
    assert M.traffic_of_layers(layers)[1]["peer_bytes"] == [0, 0] and M.traffic_of_layers(layers)[1]["sent"] == 1024
    assert M.traffic_of_layers(layers[::-1])[0]["peer_bytes"] == [0, 1024]


def test_gather_slabs_takes_every_slab_from_its_rank():
    layers = [np.full((70, 40, 4), k + 1, dtype=np.uint8) for k in range(3)]
    image = M.gather_slabs(layers, 70, 3)
    assert (image[:32] == 1).all() and (image[32:64] == 2).all() and (image[64:] == 3).all()


@pytest.mark.parametrize("world", range(1, 18))
def test_the_f32_composite_stays_within_half_a_code_of_float64(world):
    """The model's ordered "over" (f32, the kernel's operation order) against the same composite in float64 from exact code / 255 inputs, on
    premultiplied layers, where every accumulator stays in [0, 1] up to its own rounding.

    The bound. eps = 2^-24 is f32's unit roundoff: an operation whose result is at most 1 in magnitude adds at most eps of absolute error.
    With e(k) the error of the accumulator after k layers, one layer is
        src  = byte * fl(1/255)        the constant is off by a relative eps, the product by another: |error| <= 2 eps   (src <= 1)
        keep = 1 - src.a               2 eps from src.a, eps from the subtraction:                     |error| <= 3 eps
        t    = acc * keep              e(k-1) * keep + acc * 3 eps + eps of the product:               |error| <= e(k-1) + 4 eps
        acc' = src + t                 2 eps + e(k-1) + 4 eps + eps of the sum:                        e(k) <= e(k-1) + 7 eps
    so e(world) <= 7 world eps; 8 world eps below absorbs the second-order terms (accumulators that round to just above 1). The quantisation
    computes acc * 255 + 0.5 — 255 e(world), plus 255 eps for the product and 256 eps for the sum, both results being below 256 — and truncates,
    which puts the code within (-1, 0] of that; against the float64 value in code units, y = 255 acc, the code is therefore within
        0.5 + (2040 world + 511) * 2^-24
    (0.5021 at world = 17). The measured worst case is printed, not fixed in advance."""
    rng = np.random.RandomState(1700 + world)
    layers = np.stack([M.random_premultiplied(rng, 96, 64) for _ in range(world)])
    assert (layers[..., :3] <= layers[..., 3:4]).all()
    codes = M.composite(layers).astype(np.float64)
    exact = M.composite_float64(layers)
    worst = float(np.abs(codes - exact).max())
    bound = 0.5 + (2040 * world + 511) * 2.0 ** -24
    print(f"world {world}: |f32 composite - float64 composite| <= {worst:.6f} codes (bound {bound:.6f})")
    assert worst <= bound
    assert np.abs(codes - np.floor(exact + 0.5)).max() <= 1  # and never more than one code from the float64 composite's own rounding
