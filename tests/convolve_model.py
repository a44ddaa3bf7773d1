"""The model of crh_image_convolve (include/contrast_hip.h states it) in numpy, with its own wrap and its own quantisation. The sums are
int64, so an int32 overflow in the library shows as a difference. `brute` takes the definition one texel and one tap at a time, for tiny
sizes. Every test compares bytes with this; nothing here touches the library."""
import math

import numpy as np

TRANSPARENT, PAD, REPEAT, REFLECT = 0, 1, 2, 3
EDGES = (TRANSPARENT, PAD, REPEAT, REFLECT)
MAX_ORDER = 15
MAX_SUM = 1 << 22


def quantize(kernel, divisor, bias):
    """-> (k int64 [order_y, order_x], bias_k): floor(kernel / divisor * 65536 + 1/2) on the f32 values, in float64"""
    k32 = np.asarray(kernel, dtype=np.float32).astype(np.float64)
    d = float(np.float32(divisor))
    k = np.floor(k32 / d * 65536.0 + 0.5).astype(np.int64)
    assert int(np.abs(k).sum()) <= MAX_SUM, "the gain limit"
    return k, int(math.floor(float(np.float32(bias)) * 65536.0 + 0.5))


def wrap(i, n, edge):
    """PAD, REPEAT, REFLECT of integer indices (an int64 array) into [0, n), by floor division"""
    i = np.asarray(i, dtype=np.int64)
    if edge == PAD:
        return np.clip(i, 0, n - 1)
    if edge == REPEAT:
        return i - (i // n) * n
    assert edge == REFLECT
    k = i - (i // (2 * n)) * (2 * n)
    return np.where(k < n, k, 2 * n - 1 - k)


def load(pixels):
    """c = min(c, a), as int64 [h, w, 4]"""
    p = np.asarray(pixels).astype(np.int64)
    p[..., :3] = np.minimum(p[..., :3], p[..., 3:])
    return p


def unpremultiply(loaded):
    """the straight codes (255 c + a / 2) / a beside the alpha; 0 where a = 0"""
    a = loaded[..., 3:]
    safe = np.maximum(a, 1)
    out = loaded.copy()
    out[..., :3] = np.where(a > 0, (255 * loaded[..., :3] + safe // 2) // safe, 0)
    return out


def target_of(kernel, target):
    oy, ox = np.asarray(kernel).shape
    return (ox // 2, oy // 2) if target is None else (int(target[0]), int(target[1]))


def sums(pixels, kernel, divisor, bias, target, edge, preserve_alpha):
    """-> (n int64 [h, w, 4]: the window's sums with the bias and the rounding half, s: the loaded (and, with preserve_alpha, straight) texels)"""
    k, bias_k = quantize(kernel, divisor, bias)
    oy, ox = k.shape
    tx, ty = target_of(kernel, target)
    s = load(pixels)
    if preserve_alpha:
        s = unpremultiply(s)
    h, w = s.shape[:2]
    # every source row and column any window reads, taken once: apron[q, p] = the source at (p - tx, q - ty) by the edge
    y = np.arange(h + oy - 1, dtype=np.int64) - ty
    x = np.arange(w + ox - 1, dtype=np.int64) - tx
    if edge == TRANSPARENT:
        inside = ((y >= 0) & (y < h))[:, None] & ((x >= 0) & (x < w))[None, :]
        apron = s[np.clip(y, 0, h - 1)][:, np.clip(x, 0, w - 1)] * inside[:, :, None]
    else:
        apron = s[wrap(y, h, edge)][:, wrap(x, w, edge)]
    n = np.full((h, w, 4), 255 * bias_k + 32768, dtype=np.int64)
    for r in range(oy):
        for c in range(ox):
            if k[r, c] != 0:
                n += int(k[r, c]) * apron[oy - 1 - r:oy - 1 - r + h, ox - 1 - c:ox - 1 - c + w]
    return n, s


def finish(n, s, preserve_alpha):
    v = np.clip(n >> 16, 0, 255)
    out = np.empty(n.shape, dtype=np.int64)
    if preserve_alpha:
        out[..., 3] = s[..., 3]
        out[..., :3] = (v[..., :3] * s[..., 3:] + 127) // 255
    else:
        out[..., 3] = v[..., 3]
        out[..., :3] = np.minimum(v[..., :3], v[..., 3:])
    return out.astype(np.uint8)


def convolve(pixels, kernel, divisor=1.0, bias=0.0, target=None, edge=PAD, preserve_alpha=False):
    """pixels: [h, w, 4] uint8 -> [h, w, 4] uint8"""
    n, s = sums(pixels, kernel, divisor, bias, target, edge, preserve_alpha)
    assert int(np.abs(n).max()) < 2 ** 31  # the header's bound
    return finish(n, s, preserve_alpha)


def brute(pixels, kernel, divisor=1.0, bias=0.0, target=None, edge=PAD, preserve_alpha=False):
    """The definition itself, one texel and one tap at a time in Python integers: for tiny images only (the model's own check)."""
    k32 = np.asarray(kernel, dtype=np.float32)
    oy, ox = k32.shape
    tx, ty = target_of(kernel, target)
    d = float(np.float32(divisor))
    h, w = pixels.shape[:2]

    def index(i, n):
        if edge == PAD:
            return min(max(i, 0), n - 1)
        if edge == REPEAT:
            return i % n
        m = i % (2 * n)
        return m if m < n else 2 * n - 1 - m

    def texel(x, y):
        if edge == TRANSPARENT:
            if not (0 <= x < w and 0 <= y < h):
                return [0, 0, 0, 0]
        else:
            x, y = index(x, w), index(y, h)
        r, g, b, a = (int(v) for v in pixels[y, x])
        colour = [min(r, a), min(g, a), min(b, a)]
        if preserve_alpha:
            colour = [(255 * c + a // 2) // a if a else 0 for c in colour]
        return colour + [a]

    bias_k = math.floor(float(np.float32(bias)) * 65536.0 + 0.5)
    out = np.zeros((h, w, 4), dtype=np.uint8)
    for j in range(h):
        for i in range(w):
            n = [255 * bias_k + 32768] * 4
            for r in range(oy):
                for c in range(ox):
                    q = math.floor(float(k32[r, c]) / d * 65536.0 + 0.5)
                    s = texel(i - tx + (ox - 1 - c), j - ty + (oy - 1 - r))
                    for ch in range(4):
                        n[ch] += q * s[ch]
            v = [min(max(m >> 16, 0), 255) for m in n]
            if preserve_alpha:
                a = int(pixels[j, i, 3])
                out[j, i] = [(v[0] * a + 127) // 255, (v[1] * a + 127) // 255, (v[2] * a + 127) // 255, a]
            else:
                out[j, i] = [min(v[0], v[3]), min(v[1], v[3]), min(v[2], v[3]), v[3]]
    return out


def random_pixels(rng, w, h):
    """Random texels, about a quarter of them with a colour above its alpha (so the load's clamp is exercised), some transparent, some opaque"""
    a = rng.randint(0, 256, (h, w, 1))
    a[rng.uniform(size=(h, w, 1)) < 0.1] = 0
    a[rng.uniform(size=(h, w, 1)) < 0.1] = 255
    colour = np.floor(rng.uniform(0, 1, (h, w, 3)) * (a + 1)).astype(np.int64)
    over = rng.uniform(size=(h, w, 3)) < 0.08
    colour = np.where(over, rng.randint(0, 256, (h, w, 3)), colour)
    return np.concatenate([colour, a], axis=2).astype(np.uint8)


def random_kernel(rng, order_x, order_y, gain=4.0):
    """Signed f32 entries with sum |entry| about `gain` (well inside the limit of 64), and a divisor that is not 1"""
    k = rng.uniform(-1.0, 1.0, (order_y, order_x))
    divisor = float(np.float32(rng.choice([0.5, 3.0, -2.0, 1.25])))
    k = k / np.abs(k).sum() * gain * abs(divisor)
    return k.astype(np.float32), divisor
