"""The rule of crh_image_distance_field (include/contrast_hip.h states it) as a numpy model, in integers only: the inside map extended by
the edge, 2 spread + 1 shifted mins down the columns, the same along the rows with dx^2 added, and c(D2) from the integer statement in
Python integers. This is the definition that tests/test_distance_cpu.py checks against a scalar restatement and hand-derived answers, and
that the library, the mirrors and the device are compared with byte for byte."""
import functools

import numpy as np

OUTSIDE, INSIDE = 0, 1
TRANSPARENT, PAD, REPEAT, REFLECT = 0, 1, 2, 3
EDGES = (TRANSPARENT, PAD, REPEAT, REFLECT)
R, G, B, A = 0, 1, 2, 3
NONE = 1 << 30  # "no such q": above every squared distance that counts


@functools.lru_cache(maxsize=None)
def code(d2, spread):
    """c(D2): 0 for 0, otherwise the largest c in [0, 255] with (2 c - 1)^2 spread^2 <= 260100 D2 (a tie rounds up); Python integers"""
    d2, spread = int(d2), int(spread)
    if d2 == 0:
        return 0
    if d2 >= spread * spread:  # (2 * 255 - 1)^2 = 259081 <= 260100: every such D2, "none" among them, gives 255
        return 255
    return max(c for c in range(256) if (2 * c - 1) ** 2 * spread * spread <= 260100 * d2)


def byte(d2, spread, mode):
    """The result byte of one D2: 255 - c (OUTSIDE) or c (INSIDE)"""
    return code(d2, spread) if mode == INSIDE else 255 - code(d2, spread)


def wrap(i, n, edge):
    """The image-paint block's wrap(i, n) for PAD, REPEAT and REFLECT, any number of periods out"""
    if edge == PAD:
        return np.clip(i, 0, n - 1)
    if edge == REPEAT:
        return i % n
    k = i % (2 * n)
    return np.where(k < n, k, 2 * n - 1 - k)


def grows(mode, edge):
    return mode == OUTSIDE and edge == TRANSPARENT


def size(w, h, spread, mode, edge):
    g = 2 * spread if grows(mode, edge) else 0
    return w + g, h + g


def inside_map(src, channel, threshold):
    """(h, w, 4) uint8 -> (h, w) bool: the stored code of the channel, as it is, against the threshold"""
    return np.asarray(src)[..., channel] >= threshold


def extended(inside, rows, columns, edge):
    """inside(x, y) at the integer positions rows x columns (arrays of any integers): through the wrap, or false outside under TRANSPARENT"""
    h, w = inside.shape
    if edge == TRANSPARENT:
        ok = ((rows >= 0) & (rows < h))[:, None] & ((columns >= 0) & (columns < w))[None, :]
        return inside[np.clip(rows, 0, h - 1)][:, np.clip(columns, 0, w - 1)] & ok
    return inside[wrap(rows, h, edge)][:, wrap(columns, w, edge)]


def squared_distances(inside, spread, mode, edge):
    """(h, w) bool -> (h', w') int64: D2 of every texel of the result, NONE where no q lies within the window (|dx|, |dy| <= spread, which
    holds every q that can change a byte)"""
    h, w = inside.shape
    s, o = spread, (spread if grows(mode, edge) else 0)
    rows, columns = np.arange(-o - s, h + o + s), np.arange(-o - s, w + o + s)
    target = extended(inside, rows, columns, edge) != (mode == INSIDE)  # what the distance is measured to
    out_h, out_w = h + 2 * o, w + 2 * o
    column = np.full((out_h, target.shape[1]), NONE, dtype=np.int64)  # min over dy of dy^2 where the target holds
    busy = target.any(axis=0)  # (a column without a target stays NONE: nothing to shift)
    held, least = target[:, busy], np.full((out_h, int(busy.sum())), NONE, dtype=np.int64)
    for dy in range(-s, s + 1):
        np.minimum(least, np.where(held[s + dy:s + dy + out_h], dy * dy, NONE), out=least)
    column[:, busy] = least
    d2 = np.full((out_h, out_w), NONE, dtype=np.int64)
    live = (column < NONE).any(axis=1)  # (a row without a column distance stays NONE)
    rows_held, rows_least = column[live], d2[live]
    for dx in range(-s, s + 1):
        np.minimum(rows_least, rows_held[:, s + dx:s + dx + out_w] + dx * dx, out=rows_least)
    d2[live] = rows_least
    return np.minimum(d2, NONE)


def distance_field(src, spread, mode=OUTSIDE, channel=A, threshold=128, edge=TRANSPARENT):
    """(h, w, 4) uint8 -> the (h', w', 4) uint8 result"""
    src = np.asarray(src)
    assert src.dtype == np.uint8 and src.ndim == 3 and src.shape[2] == 4
    return of_inside(inside_map(src, channel, threshold), spread, mode, edge)


def of_inside(inside, spread, mode, edge):
    """The result from the inside map alone (all that the rule reads of the source)"""
    d2 = squared_distances(np.ascontiguousarray(inside, dtype=bool), spread, mode, edge)
    values, where = np.unique(d2, return_inverse=True)
    bytes_ = np.array([byte(int(v), spread, mode) for v in values], dtype=np.uint8)[where.reshape(d2.shape)]
    return np.repeat(bytes_[..., None], 4, axis=2)
