"""The rule of crh_image_transform (include/contrast_hip.h states it) as a vectorised numpy model: positions in float64 ufuncs (one
rounding per written operation, no contraction), everything behind them in integers. NEAREST and LINEAR read the source with
tests/displace_model.py's fetch and blend; CUBIC and crh_transform_fit are restated here from the header. tests/test_transform_cpu.py
checks the library against it and tests/test_gpu_transform.py the device, byte for byte."""
import math

import numpy as np

import displace_model as DM

NEAREST, LINEAR, CUBIC = 0, 1, 2
FILTERS = (NEAREST, LINEAR, CUBIC)
TRANSPARENT, PAD, REPEAT, REFLECT = DM.EDGES
EDGES = DM.EDGES
LIMIT = 2097152.0  # 2^21: what a position is clamped to
MAX_ENTRY = 2.0 ** 40


def is_affine(m):
    return m[6] == 0.0 and m[7] == 0.0 and m[8] == 1.0


def positions(matrix, width, height):
    """-> (X, Y, visible): int64 and bool arrays of (height, width); an invisible texel has position (0, 0)"""
    m = [np.float64(v) for v in np.asarray(matrix, dtype=np.float64).reshape(9)]
    j, i = np.mgrid[0:height, 0:width]
    u, v = i.astype(np.float64) + 0.5, j.astype(np.float64) + 0.5
    px, py = (m[0] * u + m[1] * v) + m[2], (m[3] * u + m[4] * v) + m[5]
    visible = np.ones((height, width), dtype=bool)
    if not is_affine(m):
        ws = (m[6] * u + m[7] * v) + m[8]
        visible = ws > 0.0
        with np.errstate(over="ignore", divide="ignore"):
            d = np.where(visible, ws, 1.0)
            px, py = px / d, py / d
    out = []
    for p in (px, py):
        p = np.where(p < -LIMIT, -LIMIT, np.where(p > LIMIT, LIMIT, p))
        out.append(np.where(visible, np.floor(p * 256.0 + 0.5), 0.0).astype(np.int64))
    assert all(np.abs(a).max() <= 2 ** 29 for a in out)
    return out[0], out[1], visible


def cubic_weights(F):
    """(c0, c1, c2, c3) of the phase F, python integers: >> is the arithmetic shift"""
    W0, W2, W3 = -F ** 3 + 512 * F ** 2 - 65536 * F, -3 * F ** 3 + 1024 * F ** 2 + 65536 * F, F ** 3 - 256 * F ** 2
    c0, c2, c3 = (W0 + 1024) >> 11, (W2 + 1024) >> 11, (W3 + 1024) >> 11
    return c0, 16384 - c0 - c2 - c3, c2, c3


CUBIC_TABLE = np.array([cubic_weights(F) for F in range(256)], dtype=np.int64)  # (256, 4)


def sample(src, X, Y, filter, edge):
    """The value at the positions (X, Y) -> int64 (..., 4)"""
    if filter == NEAREST:
        return DM.fetch(src, X >> 8, Y >> 8, edge)
    ax, ay = X - 128, Y - 128
    i0, j0 = ax >> 8, ay >> 8
    if filter == LINEAR:  # displace_model.displace's four lines
        fx, fy = (ax & 255)[..., None], (ay & 255)[..., None]
        top = DM.fetch(src, i0, j0, edge) * (256 - fx) + DM.fetch(src, i0 + 1, j0, edge) * fx
        bottom = DM.fetch(src, i0, j0 + 1, edge) * (256 - fx) + DM.fetch(src, i0 + 1, j0 + 1, edge) * fx
        return (top * (256 - fy) + bottom * fy + 32768) >> 16
    cx, cy = CUBIC_TABLE[ax & 255], CUBIC_TABLE[ay & 255]  # (..., 4)
    total = 0
    for r in range(4):
        row = sum(cx[..., k, None] * DM.fetch(src, i0 - 1 + k, j0 - 1 + r, edge) for k in range(4))
        h = (row + 32) >> 6
        assert h.min() >= -8161 and h.max() <= 73440
        total = total + cy[..., r, None] * h
    assert np.abs(total).max() <= 1372456960
    value = np.clip((total + 2 ** 21) >> 22, 0, 255)
    value[..., :3] = np.minimum(value[..., :3], value[..., 3:])
    return value


def transform(src, matrix, width, height, filter=LINEAR, edge=TRANSPARENT):
    """(sh, sw, 4) uint8 source, the result -> source matrix (9 entries) -> the (height, width, 4) uint8 result"""
    src = np.asarray(src)
    assert src.dtype == np.uint8 and src.ndim == 3 and src.shape[2] == 4
    X, Y, visible = positions(matrix, width, height)
    value = sample(src, X, Y, filter, edge)
    assert value.min() >= 0 and value.max() <= 255
    return np.where(visible[..., None], value, 0).astype(np.uint8)


def fit(width, height, forward):
    """crh_transform_fit in python floats (binary64, one rounding per operation) -> (matrix of 9, (w, h), origin), or the refusal's text"""
    a, b, c, d, e, f, g, h, i = (float(v) for v in forward)
    affine = g == 0.0 and h == 0.0 and i == 1.0
    xs, ys = [], []
    for x, y in ((0.0, 0.0), (float(width), 0.0), (0.0, float(height)), (float(width), float(height))):
        X, Y = (a * x + b * y) + c, (d * x + e * y) + f
        if not affine:
            W = (g * x + h * y) + i
            if not W > 0.0:
                return "a corner is behind the horizon"
            X, Y = X / W, Y / W
        xs.append(X), ys.append(Y)
    x0, x1, y0, y1 = math.floor(min(xs)), math.ceil(max(xs)), math.floor(min(ys)), math.ceil(max(ys))
    w, t = max(1, x1 - x0), max(1, y1 - y0)
    if w > 16384 or t > 16384:
        return "the result is outside [1, 16384]"
    A = [e * i - f * h, c * h - b * i, b * f - c * e, f * g - d * i, a * i - c * g, c * d - a * f, d * h - e * g, b * g - a * h, a * e - b * d]
    det = (a * A[0] + b * A[3]) + c * A[6]
    if det == 0.0:
        return "forward is singular"
    n = [v / det for v in A]
    if not all(math.isfinite(v) for v in n):
        return "forward is singular"
    for row in range(3):
        n[3 * row + 2] = (n[3 * row] * float(x0) + n[3 * row + 1] * float(y0)) + n[3 * row + 2]
    return n, (w, t), (-x0, -y0)


def matrices(sw, sh, w, h):
    """The result -> source matrices of the tests, by name, for a source of sw x sh and a result of w x h"""
    c, s = math.cos(math.radians(30.0)), math.sin(math.radians(30.0))
    k = 2.0 / (w + h)  # the horizon of `horizon` is the line u + v = (w + h) / 2, which crosses every result of more than one texel
    return {
        "identity": (1, 0, 0, 0, 1, 0, 0, 0, 1),
        "translate_integer": (1, 0, 3, 0, 1, -2, 0, 0, 1),
        "translate_half": (1, 0, 0.5, 0, 1, -1.5, 0, 0, 1),
        "turn_90": (0, 1, 0, -1, 0, sh, 0, 0, 1),
        "turn_180": (-1, 0, sw, 0, -1, sh, 0, 0, 1),
        "turn_270": (0, -1, sw, 1, 0, 0, 0, 0, 1),
        "rotate_30": (c, -s, sw / 2 - c * (w / 2) + s * (h / 2), s, c, sh / 2 - s * (w / 2) - c * (h / 2), 0, 0, 1),
        "scale_2.5": (2.5, 0, 0, 0, 2.5, 0, 0, 0, 1),
        "scale_0.4": (0.4, 0, 0, 0, 0.4, 0, 0, 0, 1),
        "shear": (1, 0.35, -2, -0.2, 1, 1, 0, 0, 1),
        "horizon": (1.1, 0.1, 0, -0.05, 0.9, 0.3, -k, -k, 1),
        "w_2": (1, 0, 0, 0, 1, 0, 0, 0, 2),
        "point": (0, 0, 2.3, 0, 0, 1.7, 0, 0, 1),
        "far": (1, 0, 3e6, 0, 1, -3e6, 0, 0, 1),
    }


def source(w, h, seed, premultiplied=True):
    """Random texels; not premultiplied, about four texels in ten hold a colour above their alpha"""
    px = np.random.RandomState(seed).randint(0, 256, (h, w, 4)).astype(np.uint8)
    if premultiplied:
        px[..., :3] = np.minimum(px[..., :3], px[..., 3:])
    return px


def first_mismatch(got, want):
    """None, or a text that names the first texel that differs"""
    if got.shape != want.shape:
        return f"shape {got.shape}, the model {want.shape}"
    bad = (got != want).any(axis=2)
    if not bad.any():
        return None
    at = tuple(np.argwhere(bad)[0])
    return f"{int(bad.sum())} of {bad.size} texels differ, first at (row, column) {at}: {got[at]}, the model {want[at]}"
