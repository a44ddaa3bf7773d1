"""The model of crh_image_color_filter, written from the text of include/contrast_hip.h: the six integer stages on 8-bit codes in numpy (int64
inside, with the assertion that every matrix sum fits signed 32 bits, as the header says), and — separately — the real-valued evaluation in
float64 (unpremultiply, matrix, clamp, premultiply, no rounding anywhere), with the bound on the distance between the two."""
import numpy as np

MATRIX_MAX = 16.0  # CRH_COLOR_MATRIX_MAX
I = np.int64


def f32(values):
    """20 coefficients as the library receives them: float32, [4, 5]"""
    m = np.asarray(values, dtype=np.float64).astype(np.float32).reshape(4, 5)
    return m


def coefficients(matrix):
    """k[i][j] = floor((double) m[i][j] * 65536 + 0.5); None is the identity"""
    if matrix is None:
        matrix = identity()
    m = f32(matrix).astype(np.float64)
    assert np.isfinite(m).all() and (np.abs(m) <= MATRIX_MAX).all()
    k = np.floor(m * 65536.0 + 0.5).astype(I)
    assert (np.abs(k) <= 1 << 20).all()
    return k


def load(texels):
    """[..., 4] uint8 -> int64 codes with each colour clamped to its alpha"""
    t = np.asarray(texels).astype(I)
    t[..., :3] = np.minimum(t[..., :3], t[..., 3:4])
    return t


def unpremultiply(codes):
    """u_c = (255 c + a / 2) / a for a > 0, 0 for a = 0; u_a = a"""
    a = codes[..., 3:4]
    u = codes.copy()
    u[..., :3] = np.where(a > 0, (255 * codes[..., :3] + a // 2) // np.maximum(a, 1), 0)
    assert (u <= 255).all()
    return u


def apply_matrix(u, k):
    """v_i = clamp(floor(n_i / 65536), 0, 255), n_i = sum_j k[i][j] u_j + 255 k[i][4] + 32768"""
    n = u @ k[:, :4].T + 255 * k[:, 4] + 32768
    assert (np.abs(n) < 1 << 31).all()
    return np.clip(n >> 16, 0, 255)  # (>> on int64 is arithmetic: the floor)


def apply_tables(v, tables):
    if tables is None:
        return v
    tables = np.asarray(tables, dtype=np.uint8).reshape(4, 256).astype(I)
    out = np.empty_like(v)
    for i in range(4):
        out[..., i] = tables[i][v[..., i]]
    return out


def premultiply(v):
    out = np.empty(v.shape, dtype=np.uint8)
    out[..., 3] = v[..., 3]
    out[..., :3] = (v[..., :3] * v[..., 3:4] + 127) // 255
    return out


def straight(texels, matrix=None, tables=None):
    """The straight codes after stage 5: [..., 4] int64"""
    return apply_tables(apply_matrix(unpremultiply(load(texels)), coefficients(matrix)), tables)


def texels(texels_in, matrix=None, tables=None):
    """crh_color_filter_texels / crh_image_color_filter: [..., 4] uint8 -> [..., 4] uint8"""
    return premultiply(straight(texels_in, matrix, tables))


def real(texels_in, matrix=None):
    """The real-valued filter on the loaded codes, in code units, float64: no rounding at all. [..., 4] uint8 -> [..., 4] float64"""
    t = load(texels_in).astype(np.float64)
    a = t[..., 3:4]
    with np.errstate(divide="ignore", invalid="ignore"):
        u = np.where(a > 0.0, t[..., :3] * 255.0 / a, 0.0)
    m = f32(identity() if matrix is None else matrix).astype(np.float64)
    x = np.concatenate([u, a, np.full(a.shape, 255.0)], axis=-1)
    v = np.clip(x @ m.T, 0.0, 255.0)
    out = v.copy()
    out[..., :3] = v[..., :3] * v[..., 3:4] / 255.0
    return out


def bounds(matrix):
    """(colour, alpha): the derived bound, in codes, on |texels - real| without tables.
    A straight colour u_c is within 1/2 of the real one and u_a is exact, so row i's sum is off by at most 1/2 sum_{j<3} |m_ij|; the
    coefficients are within 2^-17 of m and multiply values <= 255 (5 of them); the floor of n + 1/2 adds 1/2; the clamp does not expand.
    Hence |v_i - real| <= e_i = 1/2 (1 + sum_{j<3} |m_ij|) + 5 * 255 * 2^-17. The product v_c v_a / 255 is then off by at most
    e_c + e_a + e_c e_a / 255 (both factors <= 255), and its rounding adds 1/2."""
    m = np.abs(f32(identity() if matrix is None else matrix).astype(np.float64))
    e = 0.5 * (1.0 + m[:, :3].sum(axis=1)) + 5.0 * 255.0 * 2.0 ** -17
    colour = max(e[c] + e[3] + e[c] * e[3] / 255.0 + 0.5 for c in range(3))
    return float(colour), float(e[3])


# ---------------------------------------------------------------- the SVG filter-effects matrices, float64 -> 20 f32 values

def _rows(rows):
    return [float(np.float32(v)) for row in rows for v in row]


def identity():
    return _rows([[1, 0, 0, 0, 0], [0, 1, 0, 0, 0], [0, 0, 1, 0, 0], [0, 0, 0, 1, 0]])


def saturate(s):
    s = float(s)
    return _rows([[0.213 + 0.787 * s, 0.715 - 0.715 * s, 0.072 - 0.072 * s, 0, 0],
                  [0.213 - 0.213 * s, 0.715 + 0.285 * s, 0.072 - 0.072 * s, 0, 0],
                  [0.213 - 0.213 * s, 0.715 - 0.715 * s, 0.072 + 0.928 * s, 0, 0],
                  [0, 0, 0, 1, 0]])


def hue_rotate(degrees):
    c, s = np.cos(np.deg2rad(float(degrees))), np.sin(np.deg2rad(float(degrees)))
    return _rows([[0.213 + c * 0.787 - s * 0.213, 0.715 - c * 0.715 - s * 0.715, 0.072 - c * 0.072 + s * 0.928, 0, 0],
                  [0.213 - c * 0.213 + s * 0.143, 0.715 + c * 0.285 + s * 0.140, 0.072 - c * 0.072 - s * 0.283, 0, 0],
                  [0.213 - c * 0.213 - s * 0.787, 0.715 - c * 0.715 + s * 0.715, 0.072 + c * 0.928 + s * 0.072, 0, 0],
                  [0, 0, 0, 1, 0]])


def luminance_to_alpha():
    return _rows([[0, 0, 0, 0, 0], [0, 0, 0, 0, 0], [0, 0, 0, 0, 0], [0.2125, 0.7154, 0.0721, 0, 0]])


def flood(r, g, b, a):
    return _rows([[0, 0, 0, 0, r], [0, 0, 0, 0, g], [0, 0, 0, 0, b], [0, 0, 0, a, 0]])


def opacity(a):
    return _rows([[1, 0, 0, 0, 0], [0, 1, 0, 0, 0], [0, 0, 1, 0, 0], [0, 0, 0, a, 0]])


# ---------------------------------------------------------------- inputs

def all_pairs():
    """All 32 896 pairs c <= a as texels (c, c', c'', a) with the other two colours varied from c (still <= a): [32896, 4] uint8"""
    a, c = np.meshgrid(np.arange(256), np.arange(256), indexing="ij")
    keep = c <= a
    a, c = a[keep].astype(I), c[keep].astype(I)
    t = np.stack([c, (c * 7 + 3) % (a + 1), a - c, a], axis=1).astype(np.uint8)
    assert len(t) == 32896 and (t[:, :3] <= t[:, 3:4]).all()
    return t


def random_texels(n, seed, loose=5):
    """n random texels; every `loose`-th is left as drawn (not premultiplied), the others have rgb <= a; alphas lean to 0 and 255"""
    rng = np.random.RandomState(seed)
    t = rng.randint(0, 256, (n, 4)).astype(np.uint8)
    t[:, 3] = np.choose(rng.randint(0, 4, n), [t[:, 3], t[:, 3], 0, 255])
    tight = t.copy()
    tight[:, :3] = (tight[:, :3].astype(np.uint32) * tight[:, 3:4] + 127) // 255
    return np.where((np.arange(n) % loose == 0)[:, None], t, tight)


def random_image(rng, w, h):
    """[h, w, 4] premultiplied texels with transparent and opaque patches"""
    t = rng.randint(0, 256, (h, w, 4)).astype(np.uint8)
    t[..., 3] = np.choose(rng.randint(0, 4, (h, w)), [t[..., 3], t[..., 3], 0, 255])
    t[..., :3] = (t[..., :3].astype(np.uint32) * t[..., 3:4] + 127) // 255
    return t


def identity_tables():
    return np.tile(np.arange(256, dtype=np.uint8), 4)


def invert_tables():
    return np.tile(np.arange(255, -1, -1, dtype=np.uint8), 4)


def random_tables(seed):
    rng = np.random.RandomState(seed)
    return np.concatenate([rng.permutation(256).astype(np.uint8) for _ in range(4)])


def matrices():
    """The issue's list: (name, 20 f32 values)"""
    rng = np.random.RandomState(20)
    return [("identity", identity()), ("saturate0", saturate(0)), ("saturate2", saturate(2)), ("hue90", hue_rotate(90)), ("luminanceToAlpha", luminance_to_alpha()),
            ("flood", flood(0.2, 0.4, 0.9, 0.6)), ("random", _rows(rng.uniform(-16, 16, (4, 5)))), ("all+16", [16.0] * 20), ("all-16", [-16.0] * 20)]


def table_sets():
    return [("none", None), ("identity", identity_tables()), ("invert", invert_tables()), ("permutation", random_tables(5))]
