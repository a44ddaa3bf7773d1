"""The rule of crh_image_variable_blur (include/contrast_hip.h states it) in numpy, independent of the library and built on
tests/blur_model.py: for every level present in the mask one blur-model pass of the whole image with that level's taps, the texel's
own level selected afterwards — the definition of a gather, at the cost of one pass per level (the tests keep the levels few)."""
import numpy as np

import blur_model as B

TRANSPARENT, PAD, REPEAT, REFLECT = B.EDGES
EDGES = B.EDGES


def sigma_of(s0, s1, u):
    """The sigma of level u between s0 (code 0) and s1 (code 255), as a float32: the end points exactly, the rest one rounding of the
    stated double expression (Python floats are doubles)."""
    s0, s1 = np.float32(s0), np.float32(s1)
    if u == 0:
        return s0
    if u == 255:
        return s1
    return np.float32(float(s0) + (float(s1) - float(s0)) * float(u) / 255.0)


def _middle(total, R, n, axis, edge):
    """the n positions of a pass that belong to the source: _pass grows a TRANSPARENT axis by R on either side"""
    if edge != TRANSPARENT:
        return total
    return np.take(total, np.arange(R, R + n), axis=axis)


def _select(values, levels, sigmas, axis, edge):
    """-> per texel, the pass along `axis` with the taps of the texel's own level, unrounded (uint64)"""
    out = np.zeros(values.shape, dtype=np.uint64)
    for u in np.unique(levels):
        q, R = B.taps(sigma_of(sigmas[0], sigmas[1], int(u)))
        total = _middle(B._pass(values, q, axis, edge), R, values.shape[axis], axis, edge)
        chosen = levels == u
        out[chosen] = total[chosen]
    return out


def variable_blur(pixels, mask, sigma_x, sigma_y, channel, edge):
    """pixels, mask: [h, w, 4] uint8; sigma_x, sigma_y: (at code 0, at code 255) -> the [h, w, 4] uint8 result."""
    c = np.asarray(pixels).astype(np.uint64)
    levels = np.asarray(mask)[:, :, int(channel)]
    t = (_select(c, levels, sigma_x, 1, edge) + np.uint64(128)) >> np.uint64(8)
    assert int(t.max(initial=0)) <= 65280
    acc = _select(t, levels, sigma_y, 0, edge) + np.uint64(1 << 23)
    assert int(acc.max(initial=0)) < 1 << 32
    return (acc >> np.uint64(24)).astype(np.uint8)


# ---- the cases that the device test and the host test share: each is computed once per process

# 1 x 1; one-texel axes, which a radius of 192 wraps many times over; either side of k_image_variable_blur_h's 256-texel segment and of
# k_image_variable_blur_v's 32-row block; three segments and three row blocks with a one-texel tail in both directions
SIZES = ((1, 1), (1, 40), (40, 1), (255, 33), (257, 31), (513, 65))
LARGE = ((257, 31), (513, 65))
MASKS = ("noise", "checker", "ramp_x", "ramp_y", "uniform", "almost")
# (sigma_x, sigma_y), each (at code 0, at code 255): radius 192 and the identity in one call, ascending on x and descending on y; a small
# blur; a constant sigma; x only; y only; R = 1 with q[0] = 65536, the 17-bit tap
PAIRS = (((0.0, 64.0), (64.0, 0.0)), ((0.0, 2.5), (0.0, 2.5)), ((3.0, 3.0), (3.0, 3.0)), ((0.0, 6.0), (0.0, 0.0)), ((0.0, 0.0), (0.0, 6.0)), ((0.0, 0.01), (0.0, 0.01)))


def levels_of(w, h):
    """How many distinct levels a noise or ramp mask of this size holds: the model costs one pass per level and axis."""
    return 32 if w * h <= 4096 else 16 if w * h <= 16384 else 4


_sources, _masks, _results = {}, {}, {}


def source(w, h):
    """a random premultiplied image, fixed per size; read-only"""
    if (w, h) not in _sources:
        _sources[w, h] = B.random_premultiplied(np.random.RandomState(1000 * w + h), w, h)
        _sources[w, h].setflags(write=False)
    return _sources[w, h]


def mask(kind, w, h):
    """The mask of a kind, fixed per size, read-only: the level pattern in the channels R and A, noise in G and B.
    noise: every texel its own level (bytes quantised to levels_of values, 0 and 255 among them); checker: codes 0 and 255 alternate;
    ramp_x, ramp_y: bands from 0 to 255 along one axis, constant along the other; uniform: one value; almost: one value but for one
    texel in 64."""
    if (kind, w, h) not in _masks:
        rng = np.random.RandomState(7 * w + 13 * h + len(kind))
        n = levels_of(w, h)
        i, j = np.meshgrid(np.arange(w), np.arange(h))
        code = lambda k: np.round(k * 255.0 / (n - 1)).astype(np.uint8)  # noqa: E731
        if kind == "noise":
            level = code(rng.randint(0, n, (h, w)))
        elif kind == "checker":
            level = (((i + j) % 2) * 255).astype(np.uint8)
        elif kind == "ramp_x":
            level = code(i * n // w)
        elif kind == "ramp_y":
            level = code(j * n // h)
        elif kind == "uniform":
            level = np.full((h, w), 77, dtype=np.uint8)
        else:
            assert kind == "almost", kind
            level = np.where((i + 5 * j) % 64 == 17, 40, 200).astype(np.uint8)
        m = rng.randint(0, 256, (h, w, 4)).astype(np.uint8)
        m[..., 0] = m[..., 3] = level
        m.setflags(write=False)
        _masks[kind, w, h] = m
    return _masks[kind, w, h]


def expected(kind, w, h, pair, edge, channel):
    """the model's result of a shared case, computed once; pair indexes PAIRS"""
    key = (kind, w, h, pair, edge, channel)
    if key not in _results:
        _results[key] = variable_blur(source(w, h), mask(kind, w, h), PAIRS[pair][0], PAIRS[pair][1], channel, edge)
        _results[key].setflags(write=False)
    return _results[key]


def size_cases(w, h):
    """every edge with two masks at the hardest pair; the channels alternate"""
    return [(kind, w, h, 0, edge, 0 if (edge + k) % 2 else 3) for edge in EDGES for k, kind in enumerate(("noise", "checker"))]


def mask_cases(kind, w, h):
    """a mask with every sigma pair; the edges and the channels rotate"""
    k = MASKS.index(kind)
    return [(kind, w, h, pair, EDGES[(k + pair) % 4], 0 if (k + pair) % 2 else 3) for pair in range(len(PAIRS))]


def first_mismatch(got, want, levels):
    """-> None, or a text that names the first texel that differs, its level and both values"""
    bad = np.argwhere((got != want).any(axis=2))
    if len(bad) == 0:
        return None
    j, i = (int(v) for v in bad[0])
    return f"{len(bad)} texels differ; the first is ({i}, {j}), level {int(levels[j, i])}: got {got[j, i].tolist()}, want {want[j, i].tolist()}"
