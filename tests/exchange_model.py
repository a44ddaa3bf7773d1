"""The exact host model of the multi-GPU exchange (csrc/comm.hip), numpy only: the 16x16 tile grid, the slabs of tile rows, which tiles of a
layer are occupied, the image the exchange must produce and the bytes every rank must report to have sent. No GPU and no library call in here.

  * tile t = (t // tiles_x, t % tiles_x), tiles_x = ceil(width / 16): row-major; bit t of a rank's bitmap is word t // 32, bit t % 32;
  * rank r's slab = the tiles of the tile rows crh_comm_shard(tiles_y, r, world) gives it: a contiguous range of tile indices, empty for
    the last ranks when there are more ranks than tile rows;
  * an RGBA8 tile is occupied when any of its bytes inside the frame is non-zero — an alpha of 0 under a colour byte counts —, an RGBA16F
    tile when any half has a non-zero magnitude (-0.0 is empty);
  * the image is contrast_renderer_amd.distributed.composite_over_reference of the layers: ordered "over" in f32, one quantisation;
  * rank k sends peer p != k its occupied tiles of slab p (1024 bytes each, 2048 for RGBA16F) — crh_comm_last_peer_bytes —, and every rank
    but 0 sends rank 0 the composited tiles of its own slab, 1024 bytes for each tile ANY layer occupies — crh_comm_last_traffic's first
    figure is the sum; the second is what dense slabs would have cost: every tile outside the own slab once, and the own slab to rank 0."""
import numpy as np

from contrast_renderer_amd import distributed as D

TILE = 16
RESULT_TILE_BYTES = 1024


def tile_grid(width, height):
    """-> (tiles_x, tiles_y)"""
    return (width + TILE - 1) // TILE, (height + TILE - 1) // TILE


def n_words(width, height):
    tx, ty = tile_grid(width, height)
    return (tx * ty + 31) // 32


def tile_bytes(layer_dtype):
    return 2048 if np.dtype(layer_dtype) == np.float16 else 1024


def slab_tiles(tiles_x, tiles_y, rank, world):
    """The tiles [begin, end) of rank `rank`'s slab: whole tile rows, crh_comm_shard's split of them."""
    base, extra = divmod(tiles_y, world)
    row0 = rank * base + min(rank, extra)
    row1 = row0 + base + (1 if rank < extra else 0)
    return row0 * tiles_x, row1 * tiles_x


def pixel_nonzero(layer):
    """[height, width] bool: what the exchange calls a non-empty pixel."""
    if layer.dtype == np.float16:
        return ((np.ascontiguousarray(layer).view(np.uint16) & 0x7FFF) != 0).any(axis=2)
    assert layer.dtype == np.uint8
    return (layer != 0).any(axis=2)


def occupancy(layer):
    """[n_tiles] bool in tile order: the tiles of a [height, width, 4] layer that hold a non-empty pixel."""
    h, w = layer.shape[:2]
    tx, ty = tile_grid(w, h)
    padded = np.zeros((ty * TILE, tx * TILE), dtype=bool)
    padded[:h, :w] = pixel_nonzero(layer)
    return padded.reshape(ty, TILE, tx, TILE).any(axis=(1, 3)).reshape(-1)


def tile_pixels(occupied, width, height):
    """[height, width] bool: the pixels of the tiles `occupied` ([n_tiles] bool) names."""
    tx, ty = tile_grid(width, height)
    grid = np.asarray(occupied, dtype=bool).reshape(ty, tx)
    return np.repeat(np.repeat(grid, TILE, axis=0), TILE, axis=1)[:height, :width]


def tile_rect(tile, width, height):
    """-> (x0, y0, x1, y1): the pixels of tile `tile` that are inside the frame."""
    tx, _ = tile_grid(width, height)
    x0, y0 = (tile % tx) * TILE, (tile // tx) * TILE
    return x0, y0, min(width, x0 + TILE), min(height, y0 + TILE)


def composite(layers):
    """The image of the exchange: [world, height, width, 4] uint8 or float16 layers, rank 0 underneath -> [height, width, 4] uint8."""
    return D.composite_over_reference(np.asarray(layers))


def traffic(occupied, width, height, layer_dtype=np.uint8):
    """occupied: [world, n_tiles] bool -> for every rank dict(peer_bytes=[world], sent=, dense=): crh_comm_last_peer_bytes and
    crh_comm_last_traffic of that rank's communicator after the exchange."""
    occupied = np.asarray(occupied, dtype=bool)
    world, n_tiles = occupied.shape
    tx, ty = tile_grid(width, height)
    assert n_tiles == tx * ty
    each = tile_bytes(layer_dtype)
    union = occupied.any(axis=0)
    slabs = [slab_tiles(tx, ty, r, world) for r in range(world)]
    out = []
    for k in range(world):
        peers = [0 if p == k else int(occupied[k, b:e].sum()) * each for p, (b, e) in enumerate(slabs)]
        b, e = slabs[k]
        sent = sum(peers) + (int(union[b:e].sum()) * RESULT_TILE_BYTES if k != 0 else 0)
        dense = (n_tiles - (e - b)) * each + ((e - b) * RESULT_TILE_BYTES if k != 0 else 0)
        out.append(dict(peer_bytes=peers, sent=sent, dense=dense))
    return out


def traffic_of_layers(layers):
    """traffic() of the layers themselves ([world, height, width, 4]): what the pixel-scan path must report."""
    layers = np.asarray(layers)
    return traffic(np.stack([occupancy(layer) for layer in layers]), layers.shape[2], layers.shape[1], layers.dtype)


def gather_slabs(layers, height, world):
    """The image of crh_frame_gather_slabs: rank k's slab of pixel rows taken from layer k."""
    out = np.zeros_like(layers[0])
    for k, (r0, r1) in enumerate(D.slab_rows(height, world)):
        out[r0:r1] = layers[k][r0:r1]
    return out


def composite_float64(layers):
    """The same ordered "over" in float64 with exact code / 255 inputs, in code units and NOT quantised: [height, width, 4] float64 in [0, 255]."""
    acc = np.zeros(np.asarray(layers[0]).shape, dtype=np.float64)
    for layer in layers:
        src = layer.astype(np.float64) / 255.0 if layer.dtype == np.uint8 else layer.astype(np.float64)
        acc = src + acc * (1.0 - src[..., 3:4])
    return np.clip(acc, 0.0, 1.0) * 255.0


def random_premultiplied(rng, width, height, opaque_share=0.2):
    """Random premultiplied RGBA8: alpha uniform with a share of 255s, every colour byte <= alpha."""
    alpha = rng.randint(0, 256, (height, width))
    alpha[rng.uniform(size=(height, width)) < opaque_share] = 255
    rgb = np.floor(rng.uniform(size=(height, width, 3)) * (alpha[..., None] + 1)).astype(int)
    return np.concatenate([np.minimum(rgb, alpha[..., None]), alpha[..., None]], axis=2).astype(np.uint8)
