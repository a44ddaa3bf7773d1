"""The model of crh_image_resize (include/contrast_hip.h states it), written from the header's text and not from the library: the taps of an
axis in pure Python floats (IEEE binary64, one rounding per operation, never fused), with lighting_model's transcription of
crh_d_sincos for the Lanczos sines, and the two integer passes in numpy int64 (every sum is far inside it, so the model cannot
overflow where the library must not). `resize` also counts how often each clamp binds, how many texels min(v, alpha) changes and how many
outputs' deficits end between two taps equally near the centre, so that a test can assert that its input reaches those paths. Nothing here touches the library."""
import math

import numpy as np

from lighting_model import PI, d_sincos

BOX, TRIANGLE, CATMULL_ROM, MITCHELL, LANCZOS3 = 0, 1, 2, 3, 4
FILTERS = (BOX, TRIANGLE, CATMULL_ROM, MITCHELL, LANCZOS3)
NAMES = {BOX: "box", TRIANGLE: "triangle", CATMULL_ROM: "catmull_rom", MITCHELL: "mitchell", LANCZOS3: "lanczos3"}
SUPPORT = {BOX: 0.5, TRIANGLE: 1.0, CATMULL_ROM: 2.0, MITCHELL: 2.0, LANCZOS3: 3.0}
MAX_TAPS = 512
ONE = 16384
MAX_GAIN = 32768


class Unsupported(Exception):
    """an axis the rule refuses (CRH_ERR_UNSUPPORTED)"""


def weight(filter, x):
    a = abs(x)
    if filter == BOX:
        return 1.0 if -0.5 <= x < 0.5 else 0.0
    if filter == TRIANGLE:
        return 1.0 - a if a < 1.0 else 0.0
    if filter == CATMULL_ROM:
        if a < 1.0:
            return ((1.5 * a - 2.5) * a) * a + 1.0
        if a < 2.0:
            return ((-0.5 * a + 2.5) * a - 4.0) * a + 2.0
        return 0.0
    if filter == MITCHELL:
        if a < 1.0:
            return (((21.0 * a - 36.0) * a) * a + 16.0) / 18.0
        if a < 2.0:
            return (((-7.0 * a + 36.0) * a - 60.0) * a + 32.0) / 18.0
        return 0.0
    assert filter == LANCZOS3
    if a >= 3.0:
        return 0.0
    if a == 0.0:
        return 1.0
    p = PI * a
    s1 = d_sincos(p)[0]
    s3 = d_sincos(p / 3.0)[0]
    return ((3.0 * s1) * s3) / (p * p)


def window(n, m, filter, o):
    """-> (lo, count, c, s) of output o"""
    ratio = float(n) / float(m)
    s = ratio if ratio > 1.0 else 1.0
    c = ((o + 0.5) * float(n)) / float(m)
    reach = SUPPORT[filter] * s
    lo = max(0, int(math.floor(c - reach)))
    hi = min(n - 1, int(math.floor(c + reach)))
    return lo, hi - lo + 1, c, s


def max_count(n, m, filter):
    """the largest window of the axis (windows only: cheap at any size)"""
    return max(window(n, m, filter, o)[1] for o in range(m))


def axis_taps(n, m, filter, tally=None):
    """-> (first, count, taps): lists of m ints, m ints and m lists of signed ints. Raises Unsupported as the rule refuses. `tally`, a dict,
    has its "split_ties" raised for every output whose deficit takes one of two taps equally near the centre and leaves the other: the
    rule's "ties to the lower index" decides its taps."""
    first, count, taps = [], [], []
    for o in range(m):
        lo, k, c, s = window(n, m, filter, o)
        if k > MAX_TAPS:
            raise Unsupported(f"{NAMES[filter]} {n} -> {m}: output {o} has {k} taps")
        w = [weight(filter, (((lo + t) + 0.5) - c) / s) for t in range(k)]
        S = 0.0
        for v in w:
            S += v
        q = [int(math.floor(v / S * 16384.0 + 0.5)) for v in w]
        d = ONE - sum(q)
        if abs(d) > k:
            raise Unsupported(f"{NAMES[filter]} {n} -> {m}: output {o} has a deficit of {d} over {k} taps")
        nearest = sorted(range(k), key=lambda t: (abs(((lo + t) + 0.5) - c), t))
        if tally is not None and 0 < abs(d) < k:
            tally["split_ties"] += int(abs(((lo + nearest[abs(d) - 1]) + 0.5) - c) == abs(((lo + nearest[abs(d)]) + 0.5) - c))
        for t in nearest[:abs(d)]:
            q[t] += 1 if d > 0 else -1
        if sum(abs(v) for v in q) > MAX_GAIN:
            raise Unsupported(f"{NAMES[filter]} {n} -> {m}: output {o} has sum |q| = {sum(abs(v) for v in q)}")
        first.append(lo), count.append(k), taps.append(q)
    return first, count, taps


def _pass(values, first, count, taps, add, shift, top, counters, name):
    """One axis (axis 1 of `values`, int64 [rows, n, 4]) -> [rows, m, 4]: clamp((sum + add) >> shift, 0, top)"""
    rows, m = values.shape[0], len(first)
    out = np.empty((rows, m, 4), dtype=np.int64)
    for o in range(m):
        q = np.asarray(taps[o], dtype=np.int64)
        total = np.tensordot(values[:, first[o]:first[o] + count[o], :], q, axes=([1], [0]))
        assert np.abs(total).max(initial=0) + add < 2 ** 31  # what the library's 32 bits must hold
        t = (total + add) >> shift  # numpy's >> on int64 is arithmetic: floor
        counters[name + "_low"] += int((t < 0).sum())
        counters[name + "_high"] += int((t > top).sum())
        out[:, o, :] = np.clip(t, 0, top)
    return out


def resize(pixels, width, height, filter, counters=None):
    """pixels: (h, w, 4) uint8 -> the (height, width, 4) uint8 result. `counters`, a dict, receives h_low, h_high, v_low, v_high (the
    channel values each clamp changed), min_alpha (the colour values min(v, alpha) lowered) and split_ties (axis_taps, both axes)."""
    pixels = np.asarray(pixels)
    h, w = pixels.shape[:2]
    tally = {"h_low": 0, "h_high": 0, "v_low": 0, "v_high": 0, "min_alpha": 0, "split_ties": 0}
    fx, cx, qx = axis_taps(w, width, filter, tally)
    fy, cy, qy = axis_taps(h, height, filter, tally)
    t = _pass(pixels.astype(np.int64), fx, cx, qx, 32, 6, 65280, tally, "h")  # [h, width, 4]
    v = _pass(np.ascontiguousarray(t.transpose(1, 0, 2)), fy, cy, qy, 1 << 21, 22, 255, tally, "v").transpose(1, 0, 2)  # [height, width, 4]
    alpha = v[:, :, 3:4]
    tally["min_alpha"] = int((v[:, :, :3] > alpha).sum())
    out = np.concatenate([np.minimum(v[:, :, :3], alpha), alpha], axis=2).astype(np.uint8)
    if counters is not None:
        counters.update(tally)
    return np.ascontiguousarray(out)


def premultiplied(rng, height, width):
    """a random premultiplied RGBA8 image with transparent, opaque and partial texels"""
    a = rng.integers(0, 256, size=(height, width, 1))
    a = np.where(rng.random((height, width, 1)) < 0.2, 0, np.where(rng.random((height, width, 1)) < 0.3, 255, a))
    rgb = (rng.integers(0, 256, size=(height, width, 3)) * a + 127) // 255
    return np.concatenate([rgb, a], axis=2).astype(np.uint8)


def saturated(rng, height, width):
    """a random premultiplied image whose colours are 0 or their texel's alpha, alpha in [96, 224]: a colour channel's overshoot
    is not its alpha's, so min(v, alpha) has work to do under a filter with negative lobes"""
    a = rng.integers(96, 225, size=(height, width, 1))
    rgb = a * rng.integers(0, 2, size=(height, width, 3))
    return np.concatenate([rgb, a], axis=2).astype(np.uint8)


def checker(height, width):
    """opaque white and transparent texels in a checkerboard: the hardest edges, which bind every clamp under a filter with negative lobes"""
    on = (np.add.outer(np.arange(height), np.arange(width)) % 2 == 0)
    return np.repeat((on * 255).astype(np.uint8)[:, :, None], 4, axis=2)
