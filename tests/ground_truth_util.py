"""Float64 ground truth for the ground-truth tests: exact curves, sample positions, winding numbers and closed-form regions. Nothing here
imports product or oracle code: every region is stated as geometry (half-planes, convex polygons, discs, distances to segments), never as a
replay of the tessellation or of the fragment code."""
import numpy as np

# Segment kinds by their integer value (path.rs:15-52 order), so that this module imports nothing from the product.
LINE, INTEGRAL_QUADRATIC, INTEGRAL_CUBIC, RATIONAL_QUADRATIC, RATIONAL_CUBIC = range(5)

# Sample positions inside a pixel (x right, y down, in pixels): the pixel centre at msaa 1, the D3D / Vulkan standard 4x pattern at msaa 4.
SAMPLE_OFFSETS = {1: np.array([[0.5, 0.5]]), 4: np.array([(6, 2), (14, 6), (2, 10), (10, 14)], dtype=np.float64) / 16.0}
F32_ULP = 2.0 ** -24  # unit roundoff of binary32


def bezier_points(p0, kind, rec, t):
    """Points of one segment at parameters t (float64, direct Bernstein evaluation) -> [len(t), 2]."""
    r = np.asarray(rec, dtype=np.float64)
    p0 = np.asarray(p0, dtype=np.float64)
    if kind == LINE:
        pts, w = [p0, r[0:2]], [1.0, 1.0]
    elif kind == INTEGRAL_QUADRATIC:
        pts, w = [p0, r[0:2], r[2:4]], [1.0, 1.0, 1.0]
    elif kind == INTEGRAL_CUBIC:
        pts, w = [p0, r[0:2], r[2:4], r[4:6]], [1.0] * 4
    elif kind == RATIONAL_QUADRATIC:
        pts, w = [p0, r[1:3], r[3:5]], [1.0, r[0], 1.0]
    else:
        pts, w = [p0, r[4:6], r[6:8], r[8:10]], list(r[0:4])
    n = len(pts) - 1
    binom = {1: [1, 1], 2: [1, 2, 1], 3: [1, 3, 3, 1]}[n]
    t = np.asarray(t, dtype=np.float64)[:, None]
    basis = [b * t ** k * (1 - t) ** (n - k) * wk for k, (b, wk) in enumerate(zip(binom, w))]
    return sum(bk * pk[None, :] for bk, pk in zip(basis, pts)) / sum(basis)


def segment_end(kind, rec):
    r = np.asarray(rec, dtype=np.float64)
    return r[{LINE: 0, INTEGRAL_QUADRATIC: 2, INTEGRAL_CUBIC: 4, RATIONAL_QUADRATIC: 3, RATIONAL_CUBIC: 8}[int(kind)]:][:2]


def flatten(path, samples=400, closed=True):
    """-> [n, 2] points along the exact curve in path coordinates."""
    t = np.linspace(0.0, 1.0, samples, endpoint=False)
    out = []
    p0 = np.asarray(path.start, dtype=np.float64)
    for kind, rec in zip(path.segment_types, path.records):
        out.append(bezier_points(p0, kind, rec, t))
        p0 = segment_end(kind, rec)
    out.append(p0[None, :])
    if closed:  # the implicit closing edge back to the start (Path.from_polygon and the like end elsewhere)
        out.append(np.asarray(path.start, dtype=np.float64)[None, :])
    return np.concatenate(out)


def flatten_error(path, samples, transform, width, height):
    """Largest distance (pixels) between the exact curve and the chords of flatten(path, samples): measured at the chord midpoints'
    parameters, doubled (the sagitta of a smooth arc between the midpoint and the chord grows at most quadratically)."""
    t = (np.arange(samples) + 0.5) / samples
    worst = 0.0
    p0 = np.asarray(path.start, dtype=np.float64)
    for kind, rec in zip(path.segment_types, path.records):
        ends = bezier_points(p0, kind, rec, np.arange(samples + 1) / samples)
        mid = bezier_points(p0, kind, rec, t)
        a, b, m = (to_pixels(v, transform, width, height) for v in (ends[:-1], ends[1:], mid))
        d = b - a
        cross = np.abs(d[:, 0] * (m[:, 1] - a[:, 1]) - d[:, 1] * (m[:, 0] - a[:, 0])) / np.maximum(np.hypot(d[:, 0], d[:, 1]), 1e-30)
        worst = max(worst, float(cross.max()))
        p0 = segment_end(kind, rec)
    return 2.0 * worst


def to_pixels(points, transform, width, height=None):
    """Path coordinates -> pixel coordinates (x right, y down) through a column-major affine instance transform."""
    height = width if height is None else height
    m = np.asarray(transform, dtype=np.float64)
    x = (m[0] * points[:, 0] + m[4] * points[:, 1] + m[12]) * 0.5 + 0.5
    y = 0.5 - (m[1] * points[:, 0] + m[5] * points[:, 1] + m[13]) * 0.5
    return np.stack([x * width, y * height], axis=1)


def pixel_jacobian(transform, width, height):
    """The 2x2 linear part of path -> pixels."""
    m = np.asarray(transform, dtype=np.float64)
    return np.array([[m[0] * width * 0.5, m[4] * width * 0.5], [-m[1] * height * 0.5, -m[5] * height * 0.5]])


def to_path(pixels, transform, width, height):
    """Pixel coordinates -> path coordinates: the float64 inverse of to_pixels (mirrored and sheared transforms included)."""
    m = np.asarray(transform, dtype=np.float64)
    jac = pixel_jacobian(transform, width, height)
    origin = np.array([(m[12] * 0.5 + 0.5) * width, (0.5 - m[13] * 0.5) * height])
    return (pixels - origin) @ np.linalg.inv(jac).T


def min_pixel_scale(transform, width, height):
    """Smallest singular value of path -> pixels: a path-space distance d is at least d * this many pixels."""
    return float(np.linalg.svd(pixel_jacobian(transform, width, height), compute_uv=False).min())


def pixel_centres(size):
    c = np.arange(size) + 0.5
    return np.stack(np.meshgrid(c, c), axis=-1).reshape(-1, 2)  # row-major: y outer, x inner


def samples(width, height, msaa):
    """-> [height * width, msaa, 2] sample positions in pixels, pixels row-major."""
    y, x = np.meshgrid(np.arange(height, dtype=np.float64), np.arange(width, dtype=np.float64), indexing="ij")
    base = np.stack([x, y], axis=-1).reshape(-1, 1, 2)
    return base + SAMPLE_OFFSETS[msaa][None, :, :]


def winding_numbers(polygon, centres):
    """Brute force (centres x chords): for small cases only; winding_grid is the row-by-row evaluator."""
    a, b = polygon[:-1], polygon[1:]
    px, py = centres[:, 0:1], centres[:, 1:2]
    upward = (a[None, :, 1] <= py) & (b[None, :, 1] > py)
    downward = (a[None, :, 1] > py) & (b[None, :, 1] <= py)
    cross = (b[None, :, 0] - a[None, :, 0]) * (py - a[None, :, 1]) - (px - a[None, :, 0]) * (b[None, :, 1] - a[None, :, 1])
    return (upward & (cross > 0)).sum(axis=1) - (downward & (cross < 0)).sum(axis=1)


def winding_grid(polygons, width, height, msaa):
    """Winding numbers of every sample of a width x height frame with respect to closed polygons in pixel coordinates -> [height * width,
    msaa] int64. Row by row: each edge adds its sign at the first sample column right of where it crosses the sample row, then a prefix
    sum along the row — O(crossings + samples), not samples x chords."""
    out = np.zeros((msaa, height, width + 1), dtype=np.int64)
    for s, (ox, oy) in enumerate(SAMPLE_OFFSETS[msaa]):
        for poly in polygons:
            a, b = poly[:-1], poly[1:]
            lo, hi = np.minimum(a[:, 1], b[:, 1]), np.maximum(a[:, 1], b[:, 1])
            # sample rows y_r = r + oy with lo <= y_r < hi (half-open: a vertex on a row counts once)
            r0 = np.clip(np.ceil(lo - oy), 0, height).astype(np.int64)
            r1 = np.clip(np.ceil(hi - oy), 0, height).astype(np.int64)
            count = np.maximum(r1 - r0, 0)
            keep = count > 0
            if not keep.any():
                continue
            edge = np.repeat(np.flatnonzero(keep), count[keep])
            rows = np.arange(len(edge)) - np.repeat(np.cumsum(count[keep]) - count[keep], count[keep]) + r0[edge]
            y = rows + oy
            ea, eb = a[edge], b[edge]
            x = ea[:, 0] + (y - ea[:, 1]) * (eb[:, 0] - ea[:, 0]) / (eb[:, 1] - ea[:, 1])
            sign = np.where(eb[:, 1] > ea[:, 1], 1, -1)
            col = np.clip(np.ceil(x - ox), 0, width).astype(np.int64)  # first column whose sample lies right of the crossing
            np.add.at(out[s], (rows, col), sign)
    return np.cumsum(out[:, :, :width], axis=2).reshape(msaa, -1).T


def distance_to_polyline(polyline, centres):
    a, b = polyline[:-1], polyline[1:]
    d = b - a
    length2 = np.maximum((d * d).sum(axis=1), 1e-30)
    best = np.full(len(centres), np.inf)
    for chunk in range(0, len(a), 512):
        aa, dd, ll = a[chunk:chunk + 512], d[chunk:chunk + 512], length2[chunk:chunk + 512]
        rel = centres[:, None, :] - aa[None, :, :]
        t = np.clip((rel * dd[None]).sum(axis=2) / ll[None], 0.0, 1.0)
        diff = rel - t[..., None] * dd[None]
        best = np.minimum(best, np.sqrt((diff * diff).sum(axis=2)).min(axis=1))
    return best


def near_distance(polylines, width, height, msaa, radius):
    """Distance (pixels) of every sample to the nearest of the polylines (pixel coordinates), computed only where it is below `radius`
    (elsewhere inf): each chord is cut into pieces of at most 2 px, and each piece visits the samples of its bounding box + radius."""
    best = np.full((height * width, msaa), np.inf)
    for poly in polylines:
        a, b = poly[:-1], poly[1:]
        pieces = np.maximum(1, np.ceil(np.hypot(*(b - a).T) / 2.0)).astype(np.int64)
        k = np.repeat(np.arange(len(a)), pieces)
        f = (np.arange(len(k)) - np.repeat(np.cumsum(pieces) - pieces, pieces)) / pieces[k]
        pa = a[k] + (b[k] - a[k]) * f[:, None]
        pb = a[k] + (b[k] - a[k]) * (f + 1.0 / pieces[k])[:, None]
        span = int(np.ceil(2.0 + 2 * radius)) + 1
        x0 = np.floor(np.minimum(pa[:, 0], pb[:, 0]) - radius).astype(np.int64)
        y0 = np.floor(np.minimum(pa[:, 1], pb[:, 1]) - radius).astype(np.int64)
        for dy in range(span + 1):
            for dx in range(span + 1):
                px, py = x0 + dx, y0 + dy
                ok = (px >= 0) & (px < width) & (py >= 0) & (py < height)
                if not ok.any():
                    continue
                idx = py[ok] * width + px[ok]
                for s, off in enumerate(SAMPLE_OFFSETS[msaa]):
                    q = np.stack([px[ok], py[ok]], axis=1) + off
                    d = pb[ok] - pa[ok]
                    t = np.clip(((q - pa[ok]) * d).sum(1) / np.maximum((d * d).sum(1), 1e-30), 0.0, 1.0)
                    dist = np.hypot(*(q - pa[ok] - t[:, None] * d).T)
                    dist = np.where(dist < radius, dist, np.inf)
                    np.minimum.at(best[:, s], idx, dist)
    return best


# ---- regions: functions of path-space points [n, 2] -> signed distance (path units; > 0 inside). Every value is a lower bound of the true
# distance to the region's boundary in magnitude (exact for half-planes and discs), so excluding |sd| < eps never keeps an ambiguous sample.

def halfplane(p, normal, c):
    """{x : normal . x <= c} with a unit normal."""
    n = np.asarray(normal, dtype=np.float64)
    n = n / np.linalg.norm(n)
    return c - p @ n


def convex_polygon(p, vertices):
    """Convex polygon, vertices in either order."""
    v = np.asarray(vertices, dtype=np.float64)
    area = 0.5 * np.sum(v[:, 0] * np.roll(v[:, 1], -1) - np.roll(v[:, 0], -1) * v[:, 1])
    if area < 0:
        v = v[::-1]
    out = np.full(len(p), np.inf)
    for a, b in zip(v, np.roll(v, -1, axis=0)):
        e = b - a
        length = np.hypot(*e)
        if length == 0:
            continue
        inward = np.array([-e[1], e[0]]) / length  # counter-clockwise order: the interior lies to the left
        out = np.minimum(out, (p - a) @ inward)
    return out


def is_convex(vertices, tol=1e-12):
    v = np.asarray(vertices, dtype=np.float64)
    e = np.roll(v, -1, axis=0) - v
    cross = e[:, 0] * np.roll(e[:, 1], -1) - e[:, 1] * np.roll(e[:, 0], -1)
    return (cross >= -tol).all() or (cross <= tol).all()


def disc(p, centre, radius):
    return radius - np.hypot(*(p - np.asarray(centre, dtype=np.float64)).T)


def union(*sds):
    return np.max(np.stack(sds), axis=0)


def intersection(*sds):
    return np.min(np.stack(sds), axis=0)


def empty(p):
    return np.full(len(p), -np.inf)


def check_coverage(covered, inside, signed_distance, eps, min_near, what=""):
    """covered: [pixels] number of covered samples read from the image; inside: [pixels, msaa] model membership; signed_distance:
    [pixels, msaa] pixel distance to the model boundary (any sign). A pixel is checked when every sample lies farther than eps from the
    boundary; every checked pixel must match exactly, and at least min_near checked pixels must have a sample within 0.25 px of the
    boundary (a case cannot pass on easy pixels alone). -> the number of such near pixels."""
    d = np.abs(signed_distance)
    checked = (d > eps).all(axis=1)
    expect = inside.sum(axis=1)
    wrong = checked & (covered != expect)
    near = int((checked & (d < 0.25).any(axis=1)).sum())
    if wrong.any():
        i = np.flatnonzero(wrong)[:5]
        raise AssertionError(f"{what}: {int(wrong.sum())} pixels differ farther than eps={eps:.2e} px from the boundary; first pixels {i.tolist()}: "
                             f"covered {covered[i].tolist()}, model {expect[i].tolist()}, distance {d[i].min(axis=1).round(4).tolist()}")
    assert near >= min_near, f"{what}: only {near} checked pixels within 0.25 px of the boundary (need {min_near})"
    return near


def andrew(points, margin):
    """convex_hull.rs:6-39, Andrew's monotone chain as the reference codes it, in float64: the points sorted by (x, y), and the middle
    one of three popped while a ∨ b ∨ c <= margin, with a ∨ b ∨ c = -det[b - a, c - a] (reading A). The margin is the
    absolute ERROR_MARGIN, so points that bend the hull by less than it are dropped even where the hull is strictly convex."""
    pts = sorted(map(tuple, np.asarray(points, dtype=np.float64)))
    if len(pts) < 3:
        return np.array(pts)

    def triple(a, b, c):
        return -((b[0] - a[0]) * (c[1] - a[1]) - (b[1] - a[1]) * (c[0] - a[0]))

    hull = []
    for p in pts:
        while len(hull) > 1 and triple(hull[-2], hull[-1], p) <= margin:
            hull.pop()
        hull.append(p)
    hull.pop()
    t = len(hull) + 1
    for p in reversed(pts):
        while len(hull) > t and triple(hull[-2], hull[-1], p) <= margin:
            hull.pop()
        hull.append(p)
    hull.pop()
    return np.array(hull)


def hull_region(p, points, margin, tolerance):
    """Signed distance to the cover hull andrew(points, margin): inside only where inside both hulls built with margin -+ tolerance,
    outside only where outside both, 0 (never checked) between them — a point whose a ∨ b ∨ c lies within `tolerance` of the margin may
    be kept or dropped by f32 arithmetic."""
    lo = convex_polygon(p, andrew(points, margin + tolerance))
    hi = convex_polygon(p, andrew(points, margin - tolerance))
    return np.where((lo > 0) & (hi > 0), np.minimum(lo, hi), np.where((lo < 0) & (hi < 0), np.maximum(lo, hi), 0.0))
