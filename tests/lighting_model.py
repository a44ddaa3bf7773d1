"""The model of crh_image_lighting (include/contrast_hip.h states it) in numpy float64, written from the rule, not from the library: its own
edges, its own Sobel gradient, a scalar transcription of crh_d_sincos for the per-call constants and a vectorised transcription of
crh_d_log / crh_d_exp / crh_d_pow (include/crh_fmath.h: the same constants in the same Horner order; numpy's + - * / sqrt on float64 are
the IEEE operations, one rounding each, never fused). `svg` is the plain real-valued SVG formula with the platform's libm, for the
closeness bound. Every test compares bytes with `lighting`; nothing here touches the library."""
import math

import numpy as np

TRANSPARENT, PAD, REPEAT, REFLECT = 0, 1, 2, 3
EDGES = (TRANSPARENT, PAD, REPEAT, REFLECT)
DIFFUSE, SPECULAR = 0, 1
OPS = (DIFFUSE, SPECULAR)
DISTANT, POINT, SPOT = 0, 1, 2
LIGHTS = (DISTANT, POINT, SPOT)
PI = 3.14159265358979323846


def f32(x):
    """The float field as the library receives it, widened to double"""
    return float(np.float32(x))


def rad(d):
    return d * (PI / 180.0)


def d_sincos(a):
    """crh_d_sincos on a Python float (IEEE binary64, no fusing): Cody-Waite reduction by pi/2, Taylor on [-pi/4, pi/4]"""
    assert abs(a) <= 1048576.0
    k = float(math.floor(a * 0.63661977236758134308 + 0.5))
    pio2_hi = 1.57079632673412561417e+00
    pio2_lo = 6.07710050650619224932e-11
    r = (a - k * pio2_hi) - k * pio2_lo
    r2 = r * r
    s = 1.0 - r2 * (1.0 / 420.0)
    for d in (342.0, 272.0, 210.0, 156.0, 110.0, 72.0, 42.0, 20.0, 6.0):
        s = 1.0 - (r2 * (1.0 / d)) * s
    s = r * s
    c = 1.0 - r2 * (1.0 / 380.0)
    for d in (306.0, 240.0, 182.0, 132.0, 90.0, 56.0, 30.0, 12.0, 2.0):
        c = 1.0 - (r2 * (1.0 / d)) * c
    q = int(k) & 3
    return ((s, c), (c, -s), (-s, -c), (-c, s))[q]


def d_log(b):
    """crh_d_log on an array of positive finite normal float64"""
    b = np.ascontiguousarray(b, dtype=np.float64)
    u = b.view(np.uint64)
    e = ((u >> np.uint64(52)) & np.uint64(0x7FF)).astype(np.int64) - 1023
    m = ((u & np.uint64(0x000FFFFFFFFFFFFF)) | np.uint64(0x3FF0000000000000)).view(np.float64)
    high = m > 1.41421356237309505
    m = np.where(high, m * 0.5, m)
    e = np.where(high, e + 1, e)
    z = (m - 1.0) / (m + 1.0)
    z2 = z * z
    s = np.full(b.shape, 1.0 / 31.0)
    for d in (29.0, 27.0, 25.0, 23.0, 21.0, 19.0, 17.0, 15.0, 13.0, 11.0, 9.0, 7.0, 5.0, 3.0):
        s = 1.0 / d + z2 * s
    s = 1.0 + z2 * s
    ln2_hi = 6.93147180369123816490e-01
    ln2_lo = 1.90821492927058770002e-10
    de = e.astype(np.float64)
    return (de * ln2_hi) + ((2.0 * z) * s + de * ln2_lo)


def d_exp(y):
    """crh_d_exp on an array, |y| <= 745"""
    y = np.asarray(y, dtype=np.float64)
    n = np.floor(y * 1.44269504088896338700 + 0.5)
    ln2_hi = 6.93147180369123816490e-01
    ln2_lo = 1.90821492927058770002e-10
    r = (y - n * ln2_hi) - n * ln2_lo
    s = 1.0 + r * (1.0 / 18.0)
    for d in (17.0, 16.0, 15.0, 14.0, 13.0, 12.0, 11.0, 10.0, 9.0, 8.0, 7.0, 6.0, 5.0, 4.0, 3.0, 2.0):
        s = 1.0 + (r * (1.0 / d)) * s
    s = 1.0 + r * s
    ni = n.astype(np.int64)
    scale = ((np.clip(ni, -1000, 1000) + 1023).astype(np.uint64) << np.uint64(52)).view(np.float64)
    return np.where(ni < -1000, 0.0, np.where(ni > 1000, np.inf, s * scale))


def d_pow(b, e):
    """crh_d_pow on an array b >= 0 (finite) and a finite scalar e >= 0"""
    b = np.asarray(b, dtype=np.float64)
    e = float(e)
    if e == 0.0:
        return np.ones(b.shape)
    special = (b == 0.0) | (b == 1.0)
    y = e * d_log(np.where(special, 2.0, b))
    out = np.where(y > 700.0, np.inf, np.where(y < -745.0, 0.0, d_exp(np.clip(y, -745.0, 700.0))))
    return np.where(b == 0.0, 0.0, np.where(b == 1.0, 1.0, out))


def wrap(i, n, edge):
    """PAD, REPEAT, REFLECT of integer indices (an int64 array) into [0, n), by floor division (blur_model's and convolve_model's edges)"""
    i = np.asarray(i, dtype=np.int64)
    if edge == PAD:
        return np.clip(i, 0, n - 1)
    if edge == REPEAT:
        return i - (i // n) * n
    assert edge == REFLECT
    k = i - (i // (2 * n)) * (2 * n)
    return np.where(k < n, k, 2 * n - 1 - k)


def heights(pixels, edge):
    """-> the alpha codes with one texel of apron on every side, int64 [h + 2, w + 2]"""
    a = np.asarray(pixels)[..., 3].astype(np.int64)
    h, w = a.shape
    y, x = np.arange(-1, h + 1, dtype=np.int64), np.arange(-1, w + 1, dtype=np.int64)
    if edge == TRANSPARENT:
        inside = ((y >= 0) & (y < h))[:, None] & ((x >= 0) & (x < w))[None, :]
        return a[np.clip(y, 0, h - 1)][:, np.clip(x, 0, w - 1)] * inside
    return a[wrap(y, h, edge)][:, wrap(x, w, edge)]


def gradient(pixels, edge):
    """-> (gx, gy, A): int64 [h, w] each"""
    p = heights(pixels, edge)
    h, w = p.shape[0] - 2, p.shape[1] - 2
    at = lambda dx, dy: p[1 + dy:1 + dy + h, 1 + dx:1 + dx + w]  # noqa: E731
    gx = (at(1, -1) + 2 * at(1, 0) + at(1, 1)) - (at(-1, -1) + 2 * at(-1, 0) + at(-1, 1))
    gy = (at(-1, 1) + 2 * at(0, 1) + at(1, 1)) - (at(-1, -1) + 2 * at(0, -1) + at(1, -1))
    return gx, gy, at(0, 0)


class Light:
    """The fields of crh_lighting that describe the light and the op, as the tests pass them around"""

    def __init__(self, kind, azimuth=0.0, elevation=0.0, position=(0.0, 0.0, 0.0), points_at=(0.0, 0.0, 0.0), spot_exponent=0.0, cone_angle=0.0):
        self.kind, self.azimuth, self.elevation, self.position, self.points_at = kind, azimuth, elevation, tuple(position), tuple(points_at)
        self.spot_exponent, self.cone_angle = spot_exponent, cone_angle

    def __repr__(self):
        return f"Light({self.kind}, az {self.azimuth}, el {self.elevation}, at {self.position}, to {self.points_at}, exp {self.spot_exponent}, cone {self.cone_angle})"


def code(t):
    return np.where(t >= 1.0, 255, np.floor(np.minimum(t, 1.0) * 255.0 + 0.5).astype(np.int64))


def lighting(pixels, light, op=DIFFUSE, surface_scale=1.0, constant=1.0, specular_exponent=1.0, color=(1.0, 1.0, 1.0), edge=PAD):
    """pixels: [h, w, 4] uint8 -> [h, w, 4] uint8, by the rule in binary64"""
    s, k, se = f32(surface_scale), f32(constant), f32(specular_exponent)
    colour = [f32(c) for c in color]
    gx, gy, a = gradient(pixels, edge)
    h, w = a.shape
    nx = (s * (-gx).astype(np.float64)) / 1020.0
    ny = (s * (-gy).astype(np.float64)) / 1020.0
    nlen = np.sqrt((nx * nx + ny * ny) + 1.0)
    if light.kind == DISTANT:
        sa, ca = d_sincos(rad(f32(light.azimuth)))
        sel, cel = d_sincos(rad(f32(light.elevation)))
        lx, ly, lz = np.full((h, w), ca * cel), np.full((h, w), sa * cel), np.full((h, w), sel)
    else:
        px, py, pz = (f32(v) for v in light.position)
        i = np.arange(w, dtype=np.float64)[None, :]
        j = np.arange(h, dtype=np.float64)[:, None]
        dx = np.broadcast_to(px - (i + 0.5), (h, w))
        dy = np.broadcast_to(py - (j + 0.5), (h, w))
        dz = pz - (s * a.astype(np.float64)) / 255.0
        length = np.sqrt((dx * dx + dy * dy) + dz * dz)
        safe = np.where(length == 0.0, 1.0, length)
        lx, ly, lz = (np.where(length == 0.0, 0.0, d / safe) for d in (dx, dy, dz))
    c = [np.full((h, w), v) for v in colour]
    if light.kind == SPOT:
        ax = [f32(t) - f32(p) for t, p in zip(light.points_at, light.position)]
        alen = math.sqrt((ax[0] * ax[0] + ax[1] * ax[1]) + ax[2] * ax[2])
        sx, sy, sz = ax[0] / alen, ax[1] / alen, ax[2] / alen
        m = -((lx * sx + ly * sy) + lz * sz)
        dark = m <= 0.0
        if f32(light.cone_angle) != 0.0:
            dark = dark | (m < d_sincos(rad(f32(light.cone_angle)))[1])
        p = d_pow(np.where(dark, 1.0, m), f32(light.spot_exponent))
        c = [np.where(dark, 0.0, v * p) for v in colour]
    out = np.empty((h, w, 4), dtype=np.int64)
    if op == DIFFUSE:
        v = k * np.maximum(((nx * lx + ny * ly) + lz) / nlen, 0.0)
        for ch in range(3):
            out[..., ch] = code(v * c[ch])
        out[..., 3] = 255
    else:
        hz = lz + 1.0
        hlen = np.sqrt((lx * lx + ly * ly) + hz * hz)
        none = hlen == 0.0
        base = np.maximum(((nx * lx + ny * ly) + hz) / (nlen * np.where(none, 1.0, hlen)), 0.0)
        v = np.where(none, 0.0, k * d_pow(np.where(none, 0.0, base), se))
        for ch in range(3):
            out[..., ch] = code(v * c[ch])
        out[..., 3] = out[..., :3].max(axis=2)
    return out.astype(np.uint8)


def svg(pixels, light, op=DIFFUSE, surface_scale=1.0, constant=1.0, specular_exponent=1.0, color=(1.0, 1.0, 1.0), edge=PAD):
    """The real-valued SVG formula (feDiffuseLighting / feSpecularLighting, filter effects 1) on the same inputs with the platform's libm ->
    float64 [h, w, 4] in units of a code, before any rounding. The sample lies at the texel's centre and the edges are the library's."""
    s, k, se = f32(surface_scale), f32(constant), f32(specular_exponent)
    colour = np.array([f32(c) for c in color])
    gx, gy, a = gradient(pixels, edge)
    h, w = a.shape
    n = np.stack([-s * gx / 1020.0, -s * gy / 1020.0, np.ones((h, w))], axis=2)
    n /= np.linalg.norm(n, axis=2, keepdims=True)
    if light.kind == DISTANT:
        az, el = math.radians(f32(light.azimuth)), math.radians(f32(light.elevation))
        l = np.broadcast_to(np.array([math.cos(az) * math.cos(el), math.sin(az) * math.cos(el), math.sin(el)]), (h, w, 3))
    else:
        px, py, pz = (f32(v) for v in light.position)
        jj, ii = np.mgrid[0:h, 0:w]
        d = np.stack([px - (ii + 0.5), py - (jj + 0.5), pz - s * a / 255.0], axis=2)
        length = np.linalg.norm(d, axis=2, keepdims=True)
        l = np.where(length == 0.0, 0.0, d / np.where(length == 0.0, 1.0, length))
    c = np.broadcast_to(colour, (h, w, 3)).copy()
    if light.kind == SPOT:
        axis = np.array([f32(t) - f32(p) for t, p in zip(light.points_at, light.position)])
        axis /= math.sqrt(float(axis @ axis))
        m = -(l @ axis)
        dark = m <= 0.0
        if f32(light.cone_angle) != 0.0:
            dark |= m < math.cos(math.radians(f32(light.cone_angle)))
        c = np.where(dark[..., None], 0.0, colour * np.power(np.where(dark, 1.0, m), f32(light.spot_exponent))[..., None])
    out = np.empty((h, w, 4))
    if op == DIFFUSE:
        out[..., :3] = np.clip(k * np.maximum((n * l).sum(axis=2), 0.0)[..., None] * c, 0.0, 1.0) * 255.0
        out[..., 3] = 255.0
    else:
        half = l + np.array([0.0, 0.0, 1.0])
        hlen = np.linalg.norm(half, axis=2, keepdims=True)
        half = np.where(hlen == 0.0, 0.0, half / np.where(hlen == 0.0, 1.0, hlen))
        v = np.where(hlen[..., 0] == 0.0, 0.0, k * np.power(np.maximum((n * half).sum(axis=2), 0.0), se))
        out[..., :3] = np.clip(v[..., None] * c, 0.0, 1.0) * 255.0
        out[..., 3] = out[..., :3].max(axis=2)
    return out


def random_pixels(rng, w, h):
    """Random alpha with random colours (some above their alpha: the colours never matter), some transparent, some opaque texels"""
    a = rng.randint(0, 256, (h, w, 1))
    a[rng.uniform(size=(h, w, 1)) < 0.1] = 0
    a[rng.uniform(size=(h, w, 1)) < 0.1] = 255
    return np.concatenate([rng.randint(0, 256, (h, w, 3)), a], axis=2).astype(np.uint8)


def smooth_pixels(w, h):
    """A soft disc (a cosine fall-off from the centre): flat parts, and gradients of every size between"""
    jj, ii = np.mgrid[0:h, 0:w]
    r = np.hypot((ii + 0.5 - w / 2.0) / max(w / 2.0, 1.0), (jj + 0.5 - h / 2.0) / max(h / 2.0, 1.0))
    a = np.floor(255.0 * np.clip(1.25 - 1.5 * r, 0.0, 1.0) ** 2 * (3.0 - 2.0 * np.clip(1.25 - 1.5 * r, 0.0, 1.0)) + 0.5).astype(np.int64)
    white = np.clip(a, 0, 255)
    return np.stack([white, white // 2, white // 3, white], axis=2).astype(np.uint8)
