"""The model of crh_image_morphology (include/contrast_hip.h states it) in numpy: per channel the min or max over a rectangle, with the edge
taken by blur_model.wrap. Exact by nature: min and max do not round. Every test compares bytes with this; nothing here touches the library."""
import numpy as np

import blur_model as BM

ERODE, DILATE = 0, 1
OPS = (ERODE, DILATE)
TRANSPARENT, PAD, REPEAT, REFLECT = BM.TRANSPARENT, BM.PAD, BM.REPEAT, BM.REFLECT
EDGES = BM.EDGES
MAX_RADIUS = 192


def grows(op, edge):
    return op == DILATE and edge == TRANSPARENT


def size(w, h, op, rx, ry, edge):
    return (w + 2 * rx, h + 2 * ry) if grows(op, edge) else (w, h)


def _pass(values, op, radius, edge):
    """The window along axis 0: output o (centred on o - radius when the result grows) is the extreme of values[o - origin - radius ..
    o - origin + radius], an index outside the axis wrapped by the edge or, for TRANSPARENT, read as zero. One shifted slice per offset."""
    n = values.shape[0]
    grown = grows(op, edge)
    n_out = n + 2 * radius if grown else n
    index = np.arange(-radius, n_out + radius, dtype=np.int64) - (radius if grown else 0)
    if edge == TRANSPARENT:
        inside = (index >= 0) & (index < n)
        apron = values[np.clip(index, 0, n - 1)] * inside.reshape([-1] + [1] * (values.ndim - 1)).astype(values.dtype)
    else:
        apron = values[BM.wrap(index, n, edge)]
    pick = np.maximum if op == DILATE else np.minimum
    out = apron[0:n_out].copy()
    for k in range(1, 2 * radius + 1):
        out = pick(out, apron[k:k + n_out])
    return out


def morphology(pixels, op, rx, ry, edge):
    """pixels: [h, w, 4] uint8 -> [h', w', 4] uint8: columns within each row first, then rows (the window is a rectangle: any order)."""
    c = np.ascontiguousarray(pixels)
    assert c.dtype == np.uint8 and c.ndim == 3 and c.shape[2] == 4
    along_x = np.moveaxis(_pass(np.moveaxis(c, 1, 0), op, int(rx), edge), 0, 1)
    return np.ascontiguousarray(_pass(along_x, op, int(ry), edge))


def brute(pixels, op, rx, ry, edge):
    """The definition itself, one texel at a time: for small images only (the model's own check)."""
    h, w = pixels.shape[:2]
    ow, oh = size(w, h, op, rx, ry, edge)
    ox, oy = ((rx, ry) if grows(op, edge) else (0, 0))
    out = np.zeros((oh, ow, 4), dtype=np.uint8)
    for j in range(oh):
        for i in range(ow):
            seen = []
            for dy in range(-ry, ry + 1):
                for dx in range(-rx, rx + 1):
                    x, y = i - ox + dx, j - oy + dy
                    if edge == TRANSPARENT:
                        seen.append(pixels[y, x] if 0 <= x < w and 0 <= y < h else np.zeros(4, dtype=np.uint8))
                    else:
                        seen.append(pixels[int(BM.wrap(y, h, edge)), int(BM.wrap(x, w, edge))])
            out[j, i] = np.max(seen, axis=0) if op == DILATE else np.min(seen, axis=0)
    return out


def ramps(w, h):
    """r rising and g falling along i + j, b rising along i - j, a = 255 - r / 4, colours scaled by a: many distinct codes survive a wide window."""
    j, i = np.meshgrid(np.arange(h, dtype=np.int64), np.arange(w, dtype=np.int64), indexing="ij")
    span = max(w + h - 2, 1)
    r = (i + j) * 255 // span
    g = 255 - r
    b = (i - j + h - 1) * 255 // span
    a = 255 - r // 4
    out = np.stack([r * a // 255, g * a // 255, b * a // 255, a], axis=2)
    return out.astype(np.uint8)


def impulses(w, h, rx, ry, seed):
    """About one non-zero texel per window area, each with values of its own (premultiplied: colour <= alpha); everything else (0, 0, 0, 0)."""
    rng = np.random.RandomState(seed)
    out = np.zeros((h, w, 4), dtype=np.uint8)
    n = max(2, (w * h) // ((2 * rx + 1) * (2 * ry + 1)))
    at = rng.choice(w * h, size=min(n, w * h), replace=False)
    a = rng.randint(32, 256, len(at))
    colour = np.floor(rng.uniform(0, 1, (len(at), 3)) * (a[:, None] + 1)).astype(int)
    out.reshape(-1, 4)[at] = np.concatenate([colour, a[:, None]], axis=1).astype(np.uint8)
    return out


def holes(w, h, rx, ry, seed):
    """The complement of impulses: sparse dark texels in a 255 image, for ERODE."""
    return (255 - impulses(w, h, rx, ry, seed)).astype(np.uint8)
