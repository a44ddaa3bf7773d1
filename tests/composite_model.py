"""The model of crh_image_composite, written from the text of include/contrast_hip.h: the integer rule on 8-bit codes in numpy (unsigned 32-bit,
as the header says), the geometry of a source placed over a backdrop, and — separately — the W3C compositing-1 definitions in float64 on
unpremultiplied colours, which the integer rule must meet within half a code."""
import numpy as np

OPS = ("CLEAR", "COPY", "DST", "SRC_OVER", "DST_OVER", "SRC_IN", "DST_IN", "SRC_OUT", "DST_OUT", "SRC_ATOP", "DST_ATOP", "XOR", "PLUS")
MODES = ("NORMAL", "MULTIPLY", "SCREEN", "OVERLAY", "DARKEN", "LIGHTEN", "HARD_LIGHT", "DIFFERENCE", "EXCLUSION")
(CLEAR, COPY, DST, SRC_OVER, DST_OVER, SRC_IN, DST_IN, SRC_OUT, DST_OUT, SRC_ATOP, DST_ATOP, XOR, PLUS) = range(13)
(NORMAL, MULTIPLY, SCREEN, OVERLAY, DARKEN, LIGHTEN, HARD_LIGHT, DIFFERENCE, EXCLUSION) = range(9)

# (fa, fb) of the header's table as ((A0, A1), (B0, B1)): fa = A0 + A1 ba, fb = B0 + B1 sa
ZERO, ONE, OTHER, COMPLEMENT = (0, 0), (255, 0), (0, 1), (255, -1)
FACTORS = {CLEAR: (ZERO, ZERO), COPY: (ONE, ZERO), DST: (ZERO, ONE), SRC_OVER: (ONE, COMPLEMENT), DST_OVER: (COMPLEMENT, ONE), SRC_IN: (OTHER, ZERO),
           DST_IN: (ZERO, OTHER), SRC_OUT: (COMPLEMENT, ZERO), DST_OUT: (ZERO, COMPLEMENT), SRC_ATOP: (OTHER, COMPLEMENT), DST_ATOP: (COMPLEMENT, OTHER),
           XOR: (COMPLEMENT, COMPLEMENT), PLUS: (ONE, ONE)}
# a transparent source leaves the backdrop unchanged under these
KEEP_BACKDROP = (SRC_OVER, DST_OVER, DST_OUT, SRC_ATOP, XOR, PLUS)
U = np.uint32


def opacity_code(opacity):
    """o = floor((double)opacity * 255 + 0.5) of the f32 opacity"""
    return int(np.floor(float(np.float32(opacity)) * 255.0 + 0.5))


def load(texels):
    """[..., 4] uint8 -> uint32 codes with each colour clamped to its alpha"""
    t = np.asarray(texels).astype(U)
    t[..., :3] = np.minimum(t[..., :3], t[..., 3:4])
    return t


def fade(codes, o):
    """the opacity stage: every source code, alpha included"""
    return (codes * U(o) + U(127)) // U(255)


def term(mode, sc, sa, bc, ba):
    """T per colour channel, in units of 1 / 255^2; sc, bc: [..., 3], sa, ba: [..., 1]"""
    if mode == NORMAL:
        return sc * ba
    if mode == MULTIPLY:
        return sc * bc
    if mode == SCREEN:
        return sc * ba + bc * sa - sc * bc
    if mode == DARKEN:
        return np.minimum(sc * ba, bc * sa)
    if mode == LIGHTEN:
        return np.maximum(sc * ba, bc * sa)
    if mode == DIFFERENCE:
        p, q = sc * ba, bc * sa
        return np.maximum(p, q) - np.minimum(p, q)
    if mode == EXCLUSION:
        return sc * ba + bc * sa - U(2) * sc * bc
    assert mode in (HARD_LIGHT, OVERLAY)
    dark = U(2) * sc <= sa if mode == HARD_LIGHT else U(2) * bc <= ba
    # (the other branch, computed where it is not taken, may wrap: np.where drops it there)
    return np.where(dark, U(2) * sc * bc, sa * ba - U(2) * (ba - bc) * (sa - sc))


def blend(s, b, mode):
    """X = sc (255 - ba) + T of loaded and faded source codes s and loaded backdrop codes b: [..., 3]"""
    sc, sa, bc, ba = s[..., :3], s[..., 3:4], b[..., :3], b[..., 3:4]
    return sc * (U(255) - ba) + term(mode, sc, sa, bc, ba)


def factor(pair, other_alpha):
    k0, k1 = pair
    if k1 == 0:
        return np.full_like(other_alpha, k0)
    return other_alpha if k1 == 1 else U(255) - other_alpha


def finish(s, b, x, op):
    """The operator and the output stage -> [..., 4] uint8"""
    sa, bc, ba = s[..., 3:4], b[..., :3], b[..., 3:4]
    fa, fb = factor(FACTORS[op][0], ba), factor(FACTORS[op][1], sa)
    out = np.empty(s.shape, dtype=np.uint8)
    out[..., :3] = np.minimum(U(255), (fa * x + U(255) * fb * bc + U(32512)) // U(65025))
    out[..., 3:4] = np.minimum(U(255), (fa * sa + fb * ba + U(127)) // U(255))
    return out


def texels(source, backdrop, op, mode, o):
    """The rule on texel pairs: two [..., 4] uint8 arrays -> [..., 4] uint8"""
    s, b = fade(load(source), o), load(backdrop)
    return finish(s, b, blend(s, b, mode), op)


def place(source, w, h, x, y):
    """The source as the result sees it: [h, w, 4], result texel (i, j) = source texel (i - x, j - y), (0, 0, 0, 0) outside; any integers x, y"""
    source = np.asarray(source)
    sh, sw = source.shape[:2]
    placed = np.zeros((h, w, 4), dtype=np.uint8)
    i0, i1, j0, j1 = max(0, x), min(w, x + sw), max(0, y), min(h, y + sh)  # (Python integers: nothing wraps)
    if i0 < i1 and j0 < j1:
        placed[j0:j1, i0:i1] = source[j0 - y:j1 - y, i0 - x:i1 - x]
    return placed


def composite(backdrop, source, op, mode, o, x, y):
    """crh_image_composite: [h, w, 4] backdrop, [sh, sw, 4] source -> [h, w, 4]"""
    backdrop = np.asarray(backdrop)
    h, w = backdrop.shape[:2]
    return texels(place(source, w, h, int(x), int(y)), backdrop, op, mode, o)


# ---------------------------------------------------------------- the W3C definitions, float64, unpremultiplied

def _hard_light(cb, cs):
    return np.where(cs <= 0.5, cb * 2.0 * cs, cb + (2.0 * cs - 1.0) - cb * (2.0 * cs - 1.0))  # multiply(cb, 2 cs) : screen(cb, 2 cs - 1)


def w3c_blend(mode, cb, cs):
    """B(Cb, Cs) of compositing-1 section 'Separable blend modes'"""
    if mode == NORMAL:
        return cs
    if mode == MULTIPLY:
        return cb * cs
    if mode == SCREEN:
        return cb + cs - cb * cs
    if mode == OVERLAY:
        return _hard_light(cs, cb)
    if mode == DARKEN:
        return np.minimum(cb, cs)
    if mode == LIGHTEN:
        return np.maximum(cb, cs)
    if mode == HARD_LIGHT:
        return _hard_light(cb, cs)
    if mode == DIFFERENCE:
        return np.abs(cb - cs)
    assert mode == EXCLUSION
    return cb + cs - 2.0 * cb * cs


def w3c(s, b, op, mode):
    """The real-valued result, in code units, for loaded (and faded) source codes s and loaded backdrop codes b, [..., 4]: unpremultiply,
    Cs' = (1 - ab) Cs + ab B(Cb, Cs), co = as Fa Cs' + ab Fb Cb, ao = as Fa + ab Fb, both clamped to 1 (PLUS)."""
    s, b = np.asarray(s, dtype=np.float64) / 255.0, np.asarray(b, dtype=np.float64) / 255.0
    al_s, al_b = s[..., 3:4], b[..., 3:4]
    with np.errstate(divide="ignore", invalid="ignore"):
        cs = np.where(al_s > 0.0, s[..., :3] / al_s, 0.0)
        cb = np.where(al_b > 0.0, b[..., :3] / al_b, 0.0)
    mixed = (1.0 - al_b) * cs + al_b * w3c_blend(mode, cb, cs)
    (a0, a1), (b0, b1) = FACTORS[op]
    fa, fb = a0 / 255.0 + a1 * al_b, b0 / 255.0 + b1 * al_s
    out = np.empty(s.shape, dtype=np.float64)
    out[..., :3] = np.minimum(1.0, al_s * fa * mixed + al_b * fb * cb)
    out[..., 3:4] = np.minimum(1.0, al_s * fa + al_b * fb)
    return out * 255.0


# ---------------------------------------------------------------- inputs

CODES = (0, 1, 2, 63, 64, 127, 128, 129, 191, 254, 255)


def grid_pairs():
    """All valid (premultiplied) texel pairs with codes from CODES, one colour code replicated over the three channels: (source, backdrop), [n, 4] each"""
    valid = np.array([(c, a) for a in CODES for c in CODES if c <= a], dtype=np.uint8)
    s, b = np.repeat(valid, len(valid), axis=0), np.tile(valid, (len(valid), 1))
    return s[:, [0, 0, 0, 1]].copy(), b[:, [0, 0, 0, 1]].copy()


def random_pairs(n, seed, loose=5):
    """n random texel pairs; every `loose`-th pair is left as drawn (not premultiplied: the load clamp), the others have rgb <= a"""
    rng = np.random.RandomState(seed)
    out = []
    for _ in range(2):
        t = rng.randint(0, 256, (n, 4)).astype(np.uint8)
        # alphas lean to the ends, where the factors are 0 and 255
        t[:, 3] = np.choose(rng.randint(0, 4, n), [t[:, 3], t[:, 3], 0, 255])
        tight = t.copy()
        tight[:, :3] = (tight[:, :3].astype(np.uint32) * tight[:, 3:4] + 127) // 255
        keep = np.arange(n) % loose == 0
        out.append(np.where(keep[:, None], t, tight))
    return out[0], out[1]


def random_image(rng, w, h):
    """[h, w, 4] premultiplied texels with transparent and opaque patches"""
    t = rng.randint(0, 256, (h, w, 4)).astype(np.uint8)
    t[..., 3] = np.choose(rng.randint(0, 4, (h, w)), [t[..., 3], t[..., 3], 0, 255])
    t[..., :3] = (t[..., :3].astype(np.uint32) * t[..., 3:4] + 127) // 255
    return t
