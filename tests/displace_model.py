"""The rule of crh_image_displace (include/contrast_hip.h states it) as a vectorised numpy model, in integers only: the definition that
tests/test_displace_cpu.py checks against a scalar restatement and known answers, and that the library, the mirrors and the device are
compared with byte for byte."""
import math

import numpy as np

NEAREST, LINEAR = 0, 1
TRANSPARENT, PAD, REPEAT, REFLECT = 0, 1, 2, 3
EDGES = (TRANSPARENT, PAD, REPEAT, REFLECT)
R, G, B, A = 0, 1, 2, 3


def scale_k(scale):
    """K = (int32) floor((double) scale * 256 + 0.5) of a scale held as a float"""
    return int(math.floor(float(np.float32(scale)) * 256.0 + 0.5))


def offsets(k, u):
    """q = floor((K (2 u - 255) + 255) / 510) for straight codes u (an int or an integer array): numpy's // is the true floor"""
    return (k * (2 * np.asarray(u, dtype=np.int64) - 255) + 255) // 510


def codes(map, channel):
    """The straight code of one channel of a (h, w, 4) uint8 map: alpha as it is, a colour min(c, a) unpremultiplied, 0 for a == 0"""
    a = map[..., 3].astype(np.int64)
    if channel == A:
        return a
    c = np.minimum(map[..., channel].astype(np.int64), a)
    return np.where(a > 0, (255 * c + a // 2) // np.maximum(a, 1), 0)


def wrap(i, n, edge):
    """The image-paint block's wrap(i, n) for PAD, REPEAT and REFLECT, any number of periods out"""
    if edge == PAD:
        return np.clip(i, 0, n - 1)
    if edge == REPEAT:
        return i % n
    k = i % (2 * n)
    return np.where(k < n, k, 2 * n - 1 - k)


def fetch(src, i, j, edge):
    """S(i, j) -> int64 (..., 4)"""
    h, w = src.shape[:2]
    if edge == TRANSPARENT:
        inside = (i >= 0) & (i < w) & (j >= 0) & (j < h)
        texels = src[np.clip(j, 0, h - 1), np.clip(i, 0, w - 1)].astype(np.int64)
        return np.where(inside[..., None], texels, 0)
    return src[wrap(j, h, edge), wrap(i, w, edge)].astype(np.int64)


def displace(src, map, scale, x_channel=A, y_channel=A, filter=LINEAR, edge=TRANSPARENT):
    """(h, w, 4) uint8 source and map, scale a number or (x, y) -> the (h, w, 4) uint8 result"""
    src, map = np.asarray(src), np.asarray(map)
    assert src.shape == map.shape and src.dtype == np.uint8 and map.dtype == np.uint8
    h, w = src.shape[:2]
    sx, sy = (scale, scale) if np.isscalar(scale) else scale
    j, i = np.mgrid[0:h, 0:w].astype(np.int64)
    X = 256 * i + 128 + offsets(scale_k(sx), codes(map, x_channel))
    Y = 256 * j + 128 + offsets(scale_k(sy), codes(map, y_channel))
    if filter == NEAREST:
        return fetch(src, X >> 8, Y >> 8, edge).astype(np.uint8)
    ax, ay = X - 128, Y - 128
    i0, j0, fx, fy = ax >> 8, ay >> 8, (ax & 255)[..., None], (ay & 255)[..., None]
    top = fetch(src, i0, j0, edge) * (256 - fx) + fetch(src, i0 + 1, j0, edge) * fx
    bottom = fetch(src, i0, j0 + 1, edge) * (256 - fx) + fetch(src, i0 + 1, j0 + 1, edge) * fx
    value = (top * (256 - fy) + bottom * fy + 32768) >> 16
    assert value.min() >= 0 and value.max() <= 255
    return value.astype(np.uint8)
