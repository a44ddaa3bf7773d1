"""The integer model of crh_image_blur (include/contrast_hip.h states it): the tap rule in Python floats and integers, the wrap of an index by
each edge, and the two passes in numpy uint64. Every GPU test compares bytes with this; nothing here touches the library."""
import math

import numpy as np

TRANSPARENT, PAD, REPEAT, REFLECT = 0, 1, 2, 3
EDGES = (TRANSPARENT, PAD, REPEAT, REFLECT)
MAX_SIGMA, MAX_RADIUS = 64.0, 192


def radius_of(sigma):
    return int(math.ceil(3.0 * float(np.float32(sigma))))


def ideal_taps(sigma):
    """-> (the float64 ideals w[k] / S * 65536 for k = 0 .. R, R); sigma is the f32 value widened to double, as the library takes it."""
    s = float(np.float32(sigma))
    R = int(math.ceil(3.0 * s))
    if R == 0:
        return [65536.0], 0
    w = [math.exp(-(k * k) / (2 * s * s)) for k in range(R + 1)]
    S = w[0]
    for k in range(1, R + 1):
        S += 2 * w[k]
    return [w[k] / S * 65536 for k in range(R + 1)], R


def taps(sigma):
    """-> (q[0 .. R] as Python integers, R): the ideals rounded half up, the rounding's deficit spread over the taps next to the centre."""
    ideal, R = ideal_taps(sigma)
    q = [int(math.floor(v + 0.5)) for v in ideal]
    d = 65536 - (q[0] + 2 * sum(q[1:]))
    g = -1 if d < 0 else 1
    m = abs(d) // 2
    assert m <= R, (sigma, d, R)
    for k in range(1, m + 1):
        q[k] += g
    q[0] += d - 2 * g * m
    return q, R


def wrap(i, n, edge):
    """The image-paint block's wrap(i, n) on integer arrays, for PAD, REPEAT and REFLECT; any i."""
    i = np.asarray(i, dtype=np.int64)
    if edge == PAD:
        return np.clip(i, 0, n - 1)
    if edge == REPEAT:
        return i - n * np.floor_divide(i, n)
    assert edge == REFLECT, edge
    k = i - 2 * n * np.floor_divide(i, 2 * n)
    return np.where(k < n, k, 2 * n - 1 - k)


def _weights(q, n, edge):
    """-> the [n_out, n] uint64 matrix of one pass: row o holds, per source index, the sum of the taps q[|k|] whose index o - origin + k wraps
    onto it (R may exceed n many times over); TRANSPARENT drops what falls outside and grows n_out to n + 2 R with origin R."""
    R = len(q) - 1
    grown = edge == TRANSPARENT
    n_out = n + 2 * R if grown else n
    centres = np.arange(n_out, dtype=np.int64) - (R if grown else 0)
    weights = np.zeros((n_out, n), dtype=np.uint64)
    rows = np.arange(n_out)
    for k in range(-R, R + 1):
        index = centres + k
        if grown:
            inside = (index >= 0) & (index < n)
            np.add.at(weights, (rows[inside], index[inside]), np.uint64(q[abs(k)]))
        else:
            np.add.at(weights, (rows, wrap(index, n, edge)), np.uint64(q[abs(k)]))
    return weights


def _slices(values, q, edge):
    """The same pass along axis 0 for an axis too long for a matrix: the source gathered once with its apron, then one shifted slice per tap."""
    R, n = len(q) - 1, values.shape[0]
    grown = edge == TRANSPARENT
    n_out = n + 2 * R if grown else n
    index = np.arange(-R, n_out + R, dtype=np.int64) - (R if grown else 0)
    if grown:
        inside = (index >= 0) & (index < n)
        apron = values[np.clip(index, 0, n - 1)] * inside.reshape([-1] + [1] * (values.ndim - 1)).astype(np.uint64)
    else:
        apron = values[wrap(index, n, edge)]
    total = np.zeros((n_out,) + values.shape[1:], dtype=np.uint64)
    for k in range(-R, R + 1):
        total += np.uint64(q[abs(k)]) * apron[k + R:k + R + n_out]
    return total


def _pass(values, q, axis, edge):
    """sum_k q[|k|] values(index + k) along `axis` in uint64; the output axis grows by 2 R for TRANSPARENT (output o is centred on o - R)."""
    moved = np.moveaxis(values, axis, 0)
    n = moved.shape[0]
    if (n + 2 * len(q)) * n <= 1 << 22:
        flat = np.ascontiguousarray(moved).reshape(n, -1)
        total = np.matmul(_weights(q, n, edge), flat).reshape((-1,) + moved.shape[1:])
    else:
        total = _slices(np.ascontiguousarray(moved), q, edge)
    return np.moveaxis(total, 0, axis)


def blur(pixels, taps_x, taps_y, edge):
    """pixels: [h, w, 4] uint8 -> the blurred [h', w', 4] uint8: t = (sum qx c + 128) >> 8 along x, out = (sum qy t + 2^23) >> 24 along y."""
    c = np.asarray(pixels).astype(np.uint64)
    t = (_pass(c, [int(v) for v in taps_x], 1, edge) + np.uint64(128)) >> np.uint64(8)
    assert int(t.max(initial=0)) <= 65280
    acc = _pass(t, [int(v) for v in taps_y], 0, edge) + np.uint64(1 << 23)
    assert int(acc.max(initial=0)) < 1 << 32
    return (acc >> np.uint64(24)).astype(np.uint8)


def blur_sigma(pixels, sigma_x, sigma_y, edge):
    """blur() with the model's own taps."""
    return blur(pixels, taps(sigma_x)[0], taps(sigma_y)[0], edge)


def random_premultiplied(rng, w, h):
    a = rng.randint(0, 256, (h, w, 1))
    return np.concatenate([np.floor(rng.uniform(0, 1, (h, w, 3)) * (a + 1)).astype(int), a], axis=2).astype(np.uint8)
