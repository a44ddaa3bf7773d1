"""A numpy float64 model of crh_image_turbulence, written from the text of include/contrast_hip.h (the Turbulence block), not from
csrc/turbulence.hpp: vectorised over texels, a loop over octaves and channels, the header's parenthesisation. numpy does not contract a
product and a sum into one operation, so every float64 operation below rounds as the header says."""
import numpy as np

FRACTAL_NOISE, TURBULENCE = 0, 1
KINDS = (FRACTAL_NOISE, TURBULENCE)
MAX_OCTAVES, MAX_FREQUENCY, MAX_OFFSET = 12, 4.0, 65536.0

_tables = {}


def start(seed):
    s = int(seed)
    if s <= 0:
        s = (abs(s) % 2147483646) + 1
    if s > 2147483646:
        s = 2147483646
    return s


def rnd(s):
    r = 16807 * (s % 127773) - 2836 * (s // 127773)
    return r + 2147483647 if r <= 0 else r


def tables(seed):
    """-> (lattice: 256 int64, gradient: (4, 256, 2) float64), made once per seed and never written."""
    if seed in _tables:
        return _tables[seed]
    s = start(seed)
    gradient = np.zeros((4, 256, 2), dtype=np.float64)
    for k in range(4):
        for i in range(256):
            s = rnd(s)
            gx = np.float64((s % 512) - 256) / np.float64(256.0)
            s = rnd(s)
            gy = np.float64((s % 512) - 256) / np.float64(256.0)
            n = np.sqrt(gx * gx + gy * gy)
            if n != 0.0:
                gradient[k, i] = (gx / n, gy / n)
    lattice = np.arange(256, dtype=np.int64)
    for i in range(255, 0, -1):
        s = rnd(s)
        j = s % 256
        lattice[i], lattice[j] = lattice[j], lattice[i]
    lattice.setflags(write=False)
    gradient.setflags(write=False)
    _tables[seed] = (lattice, gradient)
    return _tables[seed]


def frequency(f, n, stitch):
    """-> (the frequency, the period P of octave 0; 0 = no wrap) of one axis of n texels; f a float64"""
    f = np.float64(f)
    if not stitch or f == 0.0:
        return f, 0
    n = np.float64(n)
    lo, hi = np.floor(n * f) / n, -np.floor(-(n * f)) / n
    with np.errstate(divide="ignore"):
        chosen = lo if f / lo < hi / f else hi
    return chosen, int(np.floor(n * chosen + np.float64(0.5)))


def wrap(i, period):
    return (i if period == 0 else np.mod(i, period)) & 255


def noise(lattice, g, vx, vy, px, py):
    """noise(k, ...) with g = G[k]; vx of shape (1, w) and vy of shape (h, 1) -> (h, w)"""
    flx, fly = np.floor(vx), np.floor(vy)
    ix, iy = flx.astype(np.int64), fly.astype(np.int64)
    rx0, ry0 = vx - flx, vy - fly
    rx1, ry1 = rx0 - 1.0, ry0 - 1.0
    bx0, bx1, by0, by1 = wrap(ix, px), wrap(ix + 1, px), wrap(iy, py), wrap(iy + 1, py)
    a0, a1 = lattice[bx0], lattice[bx1]
    b00, b10, b01, b11 = lattice[(a0 + by0) & 255], lattice[(a1 + by0) & 255], lattice[(a0 + by1) & 255], lattice[(a1 + by1) & 255]
    sx = (rx0 * rx0) * (3.0 - (2.0 * rx0))
    sy = (ry0 * ry0) * (3.0 - (2.0 * ry0))
    u = (rx0 * g[b00, 0]) + (ry0 * g[b00, 1])
    v = (rx1 * g[b10, 0]) + (ry0 * g[b10, 1])
    a = u + (sx * (v - u))
    u = (rx0 * g[b01, 0]) + (ry1 * g[b01, 1])
    v = (rx1 * g[b11, 0]) + (ry1 * g[b11, 1])
    b = u + (sx * (v - u))
    return a + (sy * (b - a))


def turbulence(width, height, base_frequency, octaves=1, seed=0, kind=TURBULENCE, stitch=False, opaque=False, offset=(0.0, 0.0)):
    """-> (height, width, 4) uint8. base_frequency: a scalar or (x, y); every float is taken through float32 first, as the C struct holds it."""
    fx, fy = (base_frequency, base_frequency) if np.isscalar(base_frequency) else base_frequency
    lattice, gradient = tables(seed)
    fx, px = frequency(np.float64(np.float32(fx)), width, stitch)
    fy, py = frequency(np.float64(np.float32(fy)), height, stitch)
    ox, oy = np.float64(np.float32(offset[0])), np.float64(np.float32(offset[1]))
    vx0 = ((ox + np.arange(width, dtype=np.float64)) * fx)[None, :]
    vy0 = ((oy + np.arange(height, dtype=np.float64)) * fy)[:, None]
    channels = 3 if opaque else 4
    codes = np.zeros((height, width, channels), dtype=np.int64)
    for k in range(channels):
        total, ratio, vx, vy = np.zeros((height, width), dtype=np.float64), np.float64(1.0), vx0, vy0
        for o in range(octaves):
            n = noise(lattice, gradient[k], vx, vy, px << o, py << o)
            total = total + ((n if kind == FRACTAL_NOISE else np.abs(n)) / ratio)
            ratio = ratio * 2.0
            vx, vy = vx * 2.0, vy * 2.0
        t = (total + 1.0) * 0.5 if kind == FRACTAL_NOISE else total
        codes[..., k] = np.where(t >= 1.0, 255, np.where(t > 0.0, np.floor(t * 255.0 + 0.5), 0.0)).astype(np.int64)
    alpha = np.full((height, width), 255, dtype=np.int64) if opaque else codes[..., 3]
    out = np.empty((height, width, 4), dtype=np.uint8)
    for c in range(3):
        out[..., c] = (codes[..., c] * alpha + 127) // 255
    out[..., 3] = alpha
    return out
