"""Joins, caps, dashes, curved strokes, the winding rule and blending against float64 mathematics — on the oracle (CPU) and on every raster
path of the HIP library (GPU). Every other GPU test compares the kernels with the oracle byte for byte, and the oracle was written from the
same reading of the reference as the kernels: a misreading both share passes all of them. Here each case is plain data plus a model that
states the expected region in closed form from the reference's definitions (stroke.rs, shaders.wgsl, renderer.rs, cited per model), so
such a misreading fails on both sides.

Orientation (reading A, pinned by KAT-J / KAT-K): a positive stroke offset moves the band to the right of the direction of
travel in y-up path coordinates; a shape whose texcoord.x is +0.5 lies on that right side.

Tolerances. A sample is only checked where its distance to the model's boundary exceeds eps (pixels). The kernels and the oracle place
every vertex in f32: a path coordinate rounded once, one f32 instance transform (two products and two sums), then edge functions evaluated
at sample positions, each step a relative error of at most 2^-24 of the magnitudes involved. With M = largest pixel coordinate + path
extent in pixels, the accumulated position error is at most a few x 2^-24 x M; F32_SLACK = 16 bounds "a few" (about 4 roundings in the
vertex, 4 in the edge function, doubled for the stroke's own offset arithmetic: normalised tangents and line intersections in f32).
Curves add the distance between the exact curve and the chords of the float64 flattening (flatten_error, measured, not chosen)."""
import math

import numpy as np
import pytest

from contrast_renderer_amd import Cap, CurveApproximation, DashInterval, DynamicStrokeOptions, Join, Path, SegmentType, StrokeOptions, batch_from_shapes

import ground_truth_util as G

F32_SLACK = 16
ERROR_MARGIN = 1e-4  # safe_float.rs: the reference's absolute tolerance of "collinear" and "anti-parallel" (stroke.rs:62,78)
TAU = 2.0 * math.pi


def f32_eps(width, height, extent_px, slack=F32_SLACK):
    """eps in pixels from the f32 magnitudes of a case (module docstring)."""
    return slack * G.F32_ULP * (max(width, height) + extent_px)


# ---------------------------------------------------------------- cases

class Case:
    """Plain data: the shapes, their instances and colours, the frame, and a model. Coverage cases draw opaque white and model(case) ->
    (inside [pixels, msaa], signed distance [pixels, msaa] in pixels, eps, min_near); colour cases model(case) -> (expected [H, W, 4]
    float64, checkable [H, W], tolerance per channel). fmt: the frame format (renderer.FORMAT_*)."""

    def __init__(self, name, shapes, transforms, width, height, msaa=1, winding_bits=8, colors=None, model=None, kind="coverage",
                 fmt=0, fills_only=False):
        self.name, self.shapes, self.width, self.height, self.msaa, self.winding_bits = name, shapes, width, height, msaa, winding_bits
        self.transforms = np.asarray(transforms, dtype=np.float32).reshape(-1, 16)
        n = len(shapes)
        self.colors = np.tile(np.float32([1, 1, 1, 1]), (n, 1)) if colors is None else np.asarray(colors, dtype=np.float32)
        if len(self.transforms) == 1 and n > 1:
            self.transforms = np.tile(self.transforms, (n, 1))
        self.model, self.kind, self.fmt, self.fills_only = model, kind, fmt, fills_only

    @property
    def batch(self):
        return batch_from_shapes(self.shapes)


def place(width, height, cx, cy, scale, rotate=0.0, mirror=False, shear=0.0):
    """One affine instance: pixels = translate(cx, cy) * rotate * shear * mirror * scale (y-up pixels), column-major mat4 in NDC."""
    c, s = math.cos(rotate), math.sin(rotate)
    lin = np.array([[c, -s], [s, c]]) @ np.array([[1.0, shear], [0.0, 1.0]]) @ np.diag([-1.0 if mirror else 1.0, 1.0]) * scale
    m = np.zeros(16)
    m[0], m[1], m[4], m[5] = 2 * lin[0, 0] / width, 2 * lin[1, 0] / height, 2 * lin[0, 1] / width, 2 * lin[1, 1] / height
    m[10], m[15] = 1.0, 1.0
    m[12], m[13] = 2.0 * cx / width - 1.0, 2.0 * cy / height - 1.0
    return m.astype(np.float32)


TRANSFORMS = {"identity": dict(), "rotated": dict(rotate=0.61), "mirrored": dict(mirror=True, rotate=-0.3), "sheared": dict(shear=0.35, rotate=0.2)}


# ---------------------------------------------------------------- stroke geometry (path space, float64)

def right(d):
    return np.array([d[1], -d[0]])


def unit(d):
    return np.asarray(d, dtype=np.float64) / np.linalg.norm(d)


def line_intersection(p, d, q, e):
    """p + t d = q + s e."""
    t = np.linalg.solve(np.stack([d, -e], axis=1), q - p)[0]
    return p + t * d


def cap_region(kind, x, y, quad=True):
    """shaders.wgsl:165-189 on the cap quad (x in [-0.5, 0.5], y in [0, 0.5], stroke.rs:270-282,444-462) -> signed distance in widths.
    The quad spans half a width, so Square (`y > 0.5`) and Butt (`y < 0`) draw nothing and Right / Left, documented as ramps a whole width
    long (path.rs:95-98), are cut at half a width: the model follows the code, as test_caps_of_a_straight_line does."""
    if not quad:  # a dash cap: the same predicates on the whole gap (shaders.wgsl:219-226), bounded across by the band only
        if kind == Cap.Square:  # `y > 0.5`: Square fills the gap beyond half a width from the dash, as coded
            return y - 0.5
        if kind == Cap.Butt:
            return -y
    quad = np.minimum(np.minimum(0.5 - np.abs(x), y), 0.5 - y) if quad else np.full(x.shape, np.inf)
    if kind in (Cap.Square, Cap.Butt):
        return np.full(x.shape, -np.inf)
    if kind == Cap.Round:
        shape = 0.5 - np.hypot(x, y)
    elif kind == Cap.Out:
        shape = (0.5 - y - np.abs(x)) / math.sqrt(2.0)
    elif kind == Cap.In:
        shape = (np.abs(x) - y) / math.sqrt(2.0)
    elif kind == Cap.Right:
        shape = (0.5 - y - x) / math.sqrt(2.0)
    else:  # Left
        shape = (x - y + 0.5) / math.sqrt(2.0)
    return np.minimum(quad, shape)


def band(p, a, b, w, offset):
    """The quad of one straight piece a -> b: lateral [(offset - 0.5) w, (offset + 0.5) w] to the right (stroke.rs:30-50)."""
    n = right(unit(b - a))
    return G.convex_polygon(p, [a + n * (offset - 0.5) * w, a + n * (offset + 0.5) * w, b + n * (offset + 0.5) * w, b + n * (offset - 0.5) * w])


def miter_corner(c, da, db, w, offset, miter_clip):
    """-> None where there is no join (collinear, or the offset puts the outer edge on the control point), else (turn_left or None for an
    exact reversal, Pprev, the corner polygon C - Pprev - (I | clip points) - Pnext); the polygon's points past the bands are the ones
    stroke.rs:89-92 adds to the proto-hull."""
    dot = float(np.clip(da @ db, -1.0, 1.0))
    if abs(dot - 1.0) <= ERROR_MARGIN:
        return None
    mc = miter_clip * w
    if abs(dot + 1.0) <= ERROR_MARGIN:
        n = right(da)
        return None, c + n * 0.5 * w, [c - n * 0.5 * w, c + n * 0.5 * w, c + n * 0.5 * w + da * mc, c - n * 0.5 * w + da * mc]
    turn_left = da[0] * db[1] - da[1] * db[0] > 0  # (y up) the outer corner is on the right of a left turn
    side = (offset + (0.5 if turn_left else -0.5)) * w
    if abs(side) < 1e-12:
        return None
    pa, pb = c + right(da) * side, c + right(db) * side
    tip = line_intersection(pa, da, pb, db)
    if np.linalg.norm(tip - c) > mc:
        bis = unit(right(da) + right(db)) * (1.0 if turn_left else -1.0)
        qa = line_intersection(pa, da, c + bis * mc, right(bis))
        qb = line_intersection(pb, db, c + bis * mc, right(bis))
        return turn_left, pa, [c, pa, qa, qb, pb]
    return turn_left, pa, [c, pa, tip, pb]


def join_region(p, c, da, db, w, offset, miter_clip, join, dash=None, s0=0.0):
    """The join at control point c from direction da to db (stroke.rs:53-87, shaders.wgsl:191-203,287-299) -> signed distance (path units).
    Geometry: the corner between the two bands' outer edges, C - Pprev - I - Pnext, where Pprev / Pnext are the outer edge points of the
    offset band at c and I the miter point where the outer edges meet; when |I - c| > miter_clip * w (stroke.rs:66,76: miter_clip scaled by
    the width, distance from the CONTROL point) or the turn is an exact reversal, the corner is cut by the line perpendicular to the
    bisector at miter_clip * w from c. Round keeps the part within w / 2 of the control point (`radius <= 0.5`, radius = |texcoord.xy| in
    widths from c). Bevel keeps nothing: `joint()` returns the vertex's bevel bit, and stroke.rs:104-112 never sets it on joint vertices
    (only the end cap's vertices carry 0x10000, stroke.rs:448,457) — the reference draws no join at all for Bevel, reproduced as coded."""
    corner = miter_corner(c, da, db, w, offset, miter_clip)
    if corner is None or join == Join.Bevel:
        return G.empty(p)
    turn_left, pa, poly = corner
    if turn_left is None:  # (exact reversal: offset 0 only — which edge is "outer" then hangs on the sign of a zero cross product, stroke.rs:64)
        assert offset == 0.0 and dash is None
        out = G.convex_polygon(p, poly)
    else:
        assert G.is_convex(poly), "case outside the model's stated geometry (the clip line must lie beyond the bevel edge)"
        out = G.convex_polygon(p, poly)
        if dash is not None:  # the wedge's path coordinate: the join's start + the angle from Pprev's direction / tau (shaders.wgsl:296)
            rel = p - c
            e1 = unit(pa - c)
            e2 = np.array([-e1[1], e1[0]]) * (1.0 if turn_left else -1.0)  # rotating from Pprev towards Pnext
            theta = np.arctan2(rel @ e2, rel @ e1)
            radius = np.hypot(rel[:, 0], rel[:, 1])
            # a difference of pos in the wedge is an arc: tau * radius path units per unit of pos
            weight = dash[2] if len(dash) > 2 else 1.0
            out = G.intersection(out, dashed_fill(radius / w, s0 / w + theta / TAU, dash[0], dash[1], weight * TAU * radius / w) * w)
    if join == Join.Round:
        out = G.intersection(out, G.disc(p, c, 0.5 * w))
    return out


def cap_at(p, kind, at, outward, travel, w, offset):
    n = right(travel)
    origin = at + n * offset * w  # texcoord.x is +-0.5 on the offset band's edges (stroke.rs:36-49)
    rel = p - origin
    return cap_region(kind, rel @ n / w, rel @ outward / w) * w


def dash_position(pos, pattern, phase):
    """Dashed { pattern, phase } at the path coordinate `pos` (widths; shaders.wgsl:205-231, the pattern layout of renderer.rs:31-49):
    -> (gap index or -1 in a dash, distance into the gap from its start, distance to its end, distance to the nearest dash boundary)."""
    starts = np.array([d.gap_start for d in pattern])
    ends = np.array([d.gap_end for d in pattern])
    length = ends[-1]
    x = np.mod(pos - phase, length)
    gap = np.full(x.shape, -1)
    into, left = np.zeros(x.shape), np.zeros(x.shape)
    for i in range(len(pattern)):
        g = (x > starts[i]) & (x < ends[i])
        gap[g], into[g], left[g] = i, x[g] - starts[i], ends[i] - x[g]
    bounds = np.concatenate([starts, ends])
    nearest = np.min(np.abs(((x[:, None] - bounds[None, :]) + 0.5 * length) % length - 0.5 * length), axis=1)
    return gap, into, left, nearest


def dashed_fill(x, pos, pattern, phase, scale):
    """Dash membership at cap coordinate x and path coordinate pos -> signed distance in widths. In gap i the dash before it ends with
    pattern[i].dash_end, tested at the distance into the gap, and the dash after it starts with pattern[i + 1].dash_start, tested at the
    distance to the gap's end (renderer.rs:45-46 packs them so, shaders.wgsl:219-226 reads them). `scale`: widths of distance per unit of pos."""
    scale = np.broadcast_to(np.asarray(scale, dtype=np.float64), pos.shape)
    gap, into, left, nearest = dash_position(pos, pattern, phase)
    out = nearest * scale
    for i, d in enumerate(pattern):
        g = gap == i
        a = np.maximum(cap_region(d.dash_end, x[g], into[g], quad=False) * np.minimum(scale[g], 1.0), -into[g] * scale[g])
        b = np.maximum(cap_region(pattern[(i + 1) % len(pattern)].dash_start, x[g], left[g], quad=False) * np.minimum(scale[g], 1.0), -left[g] * scale[g])
        out[g] = np.maximum(a, b)
    return out


def polyline_parts(pts, w, offset, miter_clip, closed, join, start, end, dash=None):
    """Solid or dashed stroke of a polyline (Line segments) as parts [(path-space points bounding the part, fn(p) -> sd)]: bands, joins
    (interior vertices, and every vertex of a closed path: the closing join, stroke.rs:423-432), caps at the ends of an open path on
    half-width quads behind the start and beyond the end (stroke.rs:270-282,444-462). dash = (pattern, phase): every part runs through the
    pattern test instead of the cap test (shaders.wgsl:272-274,295-297) at path coordinate pos (widths) = the length so far, plus
    acos(dot) / 2 pi per join (stroke.rs:111), and inside a join's wedge pos = the join's start + atan2 / tau (shaders.wgsl:296)."""
    pts = [np.asarray(v, dtype=np.float64) for v in pts]
    segs = list(zip(pts[:-1], pts[1:])) + ([(pts[-1], pts[0])] if closed else [])
    dirs = [unit(b - a) for a, b in segs]
    parts, s = [], 0.0
    for k, (a, b) in enumerate(segs):
        if k > 0 or closed:
            da, db = dirs[k - 1], dirs[k]
            dot = float(np.clip(da @ db, -1.0, 1.0))
            jf = (lambda c, da, db, s0: lambda p: join_region(p, c, da, db, w, offset, miter_clip, join, dash, s0))(a, da, db, s)
            parts.append((([a], w * (miter_clip + 1.0)), jf))
            if abs(dot - 1.0) > ERROR_MARGIN:
                s += math.acos(dot) / TAU * w
        u = dirs[k]
        a0 = a - u * 0.5 * w if (dash and k == 0 and not closed) else a
        b0 = b + u * 0.5 * w if (dash and k == len(segs) - 1 and not closed) else b
        parts.append((([a0, b0], w), (lambda a, u, a0, b0, s0: lambda p: band_part(p, a, u, a0, b0, w, offset, dash, s0))(a, u, a0, b0, s)))
        s += float(np.linalg.norm(b - a))
    if not closed and not dash:
        for kind, at, outward, travel in ((start, pts[0], -dirs[0], dirs[0]), (end, pts[-1], dirs[-1], dirs[-1])):
            parts.append((([at], w), (lambda kind, at, outward, travel: lambda p: cap_at(p, kind, at, outward, travel, w, offset))(kind, at, outward, travel)))
    return parts


def polyline_hull_points(pts, w, offset, miter_clip, closed):
    """The proto-hull of a polyline stroke: every vertex of the bands and of the cap quads of an open path (cut_stroke_polygon,
    stroke.rs:123-126) and each join's miter point or its two clip points (stroke.rs:89-92), whatever the join kind."""
    pts = [np.asarray(v, dtype=np.float64) for v in pts]
    segs = list(zip(pts[:-1], pts[1:])) + ([(pts[-1], pts[0])] if closed else [])
    dirs = [unit(b - a) for a, b in segs]
    out = []
    for k, (a, b) in enumerate(segs):
        u, n = dirs[k], right(dirs[k])
        ends = [a, b] + ([a - u * 0.5 * w] if k == 0 and not closed else []) + ([b + u * 0.5 * w] if k == len(segs) - 1 and not closed else [])
        out += [q + n * lat * w for q in ends for lat in (offset - 0.5, offset + 0.5)]
        if k > 0 or closed:
            corner = miter_corner(a, dirs[k - 1], u, w, offset, miter_clip)
            if corner is not None:
                out += corner[2][2:4] if corner[0] is None else corner[2][2:-1]
    return out


def hull_tolerance(points):
    """f32 error of the reference's a ∨ b ∨ c (convex_hull.rs:15-19) on vertices of magnitude <= R: the product of two differences of
    size <= 2R rounded a few times (4 x 2^-24 x 4R^2) plus the vertices' own placement error (F32_SLACK x 2^-24 x R, times 2 x 2R),
    bounded by 128 x 2^-24 x R^2."""
    r = float(np.abs(np.asarray(points)).max())
    return 128 * G.F32_ULP * r * r


def band_part(p, a, u, a0, b0, w, offset, dash, s0):
    out = band(p, a0, b0, w, offset)
    if dash:
        rel = p - a
        x = rel @ right(u) / w - offset
        out = G.intersection(out, dashed_fill(x, (s0 + rel @ u) / w, dash[0], dash[1], dash[2] if len(dash) > 2 else 1.0) * w)
    return out


def stroke_case_shape(pts, w, offset, miter_clip, closed, dynamic, approx=None):
    path = Path.from_polygon(pts) if closed else Path(start=tuple(pts[0]))
    if not closed:
        for v in pts[1:]:
            path.push_line(tuple(v))
    path.stroke_options = StrokeOptions(w, offset, miter_clip, closed, 0, approx or CurveApproximation.UniformlySpacedParameters(1))
    return [dynamic], [path]


def f32_points(pts):
    return [tuple(float(v) for v in np.float32(q)) for q in pts]


def eval_parts(case, parts):
    """Signed distance (pixels, lower bound) of the union of parts at every sample of shape 0's frame -> [P, S]: each part is evaluated
    only at the samples of its pixel bounding box (+ 2 px); elsewhere it is at least 2 px away, which counts as -2 (outside, checked)."""
    t = case.transforms[0]
    scale = G.min_pixel_scale(t, case.width, case.height)
    pix = G.samples(case.width, case.height, case.msaa)
    out = np.full(pix.shape[:2], -2.0)
    for points, fn in parts:
        if isinstance(points, tuple):  # (centre points, radius): the square around each
            pts, r = np.asarray(points[0], dtype=np.float64).reshape(-1, 2), points[1]
            pts = (pts[:, None, :] + np.array([(-r, -r), (-r, r), (r, -r), (r, r)])[None]).reshape(-1, 2)
        else:
            pts = np.asarray(points, dtype=np.float64).reshape(-1, 2)
        q = G.to_pixels(pts, t, case.width, case.height)
        x0, y0 = np.floor(q.min(axis=0) - 2).astype(int)
        x1, y1 = np.ceil(q.max(axis=0) + 2).astype(int)
        x0, y0, x1, y1 = max(x0, 0), max(y0, 0), min(x1, case.width), min(y1, case.height)
        if x0 >= x1 or y0 >= y1:
            continue
        idx = (np.arange(y0, y1)[:, None] * case.width + np.arange(x0, x1)[None, :]).reshape(-1)
        sub = pix[idx].reshape(-1, 2)
        sd = fn(G.to_path(sub, t, case.width, case.height)).reshape(len(idx), case.msaa) * scale
        out[idx] = np.maximum(out[idx], sd)
    return out


def parts_model(parts, extent_px, min_near, eps=None, hull=None):
    """Coverage of the union of parts, cut by the cover hull: the colour cover of a Shape is the strip of andrew() over its proto-hull
    (renderer.rs:736-754, convex_hull.rs), and a stencilled sample outside it stays uncovered. With the absolute ERROR_MARGIN the hull
    drops points that bend it by less than 1e-4 (in path units squared) — on a finely sampled curve or a path of many short segments that
    cuts visibly into the stroke; the model keeps that, as coded."""
    def model(case):
        sd = eval_parts(case, parts)
        if hull is not None:
            p = G.to_path(G.samples(case.width, case.height, case.msaa).reshape(-1, 2), case.transforms[0], case.width, case.height)
            flat = sd.reshape(-1)
            at = np.flatnonzero(flat >= 0)
            h = G.hull_region(p[at], hull, ERROR_MARGIN, hull_tolerance(hull)) * G.min_pixel_scale(case.transforms[0], case.width, case.height)
            flat[at] = np.minimum(flat[at], h)
            sd = flat.reshape(sd.shape)
        return sd > 0, sd, eps if eps is not None else f32_eps(case.width, case.height, extent_px), min_near
    return model


# ---- A. joins

def turn_polyline(angle_deg, left):
    """Three points: in along +x, then a turn of angle_deg to the left or right, segments of length 1."""
    a = math.radians(angle_deg) * (1 if left else -1)
    return f32_points([(-1.0, 0.0), (0.0, 0.0), (math.cos(a), math.sin(a))])


def join_cases():
    out = []
    size, scale, w = 192, 70.0, 0.36
    specs = []
    for join, clip in ((Join.Miter, 4.0), (Join.Miter, 1.1), (Join.Bevel, 4.0), (Join.Round, 4.0), (Join.Round, 0.42)):
        for angle in (5.0, 40.0, 90.0, 135.0, 179.0):
            if join == Join.Round and clip < 0.5 and angle < 90.0:
                continue  # (the clip line would cross the bevel edge: outside the geometry join_region states)
            specs.append((join, clip, angle))
    for i, (join, clip, angle) in enumerate(specs):
        left = i % 2 == 0
        offset = (-0.5, -0.2, 0.0, 0.3, 0.5)[(i * 3) % 5]
        if join == Join.Round and clip < 0.5:
            offset = 0.0  # (an offset moves the outer edge points past a clip line this close)
        tname = list(TRANSFORMS)[i % 4]
        pts = turn_polyline(angle, left)
        t = place(size, size, size / 2 + 3.3, size / 2 - 1.7, scale, **TRANSFORMS[tname])
        parts = polyline_parts(pts, w, offset, clip, False, join, Cap.Butt, Cap.Butt)
        out.append(Case(f"join-{join.name}-clip{clip}-{angle:g}deg-{'L' if left else 'R'}-off{offset}-{tname}",
                        [stroke_case_shape(pts, w, offset, clip, False, DynamicStrokeOptions.Solid(join, Cap.Butt, Cap.Butt))],
                        t, size, size, msaa=(1, 4)[i % 3 == 2], model=parts_model(parts, 3 * scale, 40, hull=polyline_hull_points(pts, w, offset, clip, False))))
    for join in (Join.Miter, Join.Round):  # exact reversal (anti_parallel, stroke.rs:78-84)
        pts = f32_points([(-1.0, 0.125), (0.5, 0.125), (-0.625, 0.125)])
        parts = polyline_parts(pts, w, 0.0, 0.8, False, join, Cap.Butt, Cap.Butt)
        out.append(Case(f"join-{join.name}-reversal", [stroke_case_shape(pts, w, 0.0, 0.8, False, DynamicStrokeOptions.Solid(join, Cap.Butt, Cap.Butt))],
                        place(size, size, size / 2, size / 2, scale, rotate=0.4), size, size, model=parts_model(parts, 3 * scale, 20, hull=polyline_hull_points(pts, w, 0.0, 0.8, False))))
    pts = f32_points([(-1.0, -0.5), (-0.2, -0.1), (0.6, 0.3), (1.0, 0.5)])  # collinear: no join (stroke.rs:62-64)
    out.append(Case("join-collinear", [stroke_case_shape(pts, w, 0.2, 4.0, False, DynamicStrokeOptions.Solid(Join.Miter, Cap.Butt, Cap.Butt))],
                    place(size, size, size / 2, size / 2, scale), size, size,
                    model=parts_model(polyline_parts(pts, w, 0.2, 4.0, False, Join.Miter, Cap.Butt, Cap.Butt), 3 * scale, 40,
                                     hull=polyline_hull_points(pts, w, 0.2, 4.0, False))))
    # closed polygons: every corner joined, the closing join included; both orientations
    for join, clip, off, rev in ((Join.Miter, 4.0, 0.3, False), (Join.Miter, 1.2, -0.2, True), (Join.Round, 4.0, 0.0, False), (Join.Round, 0.45, 0.0, True)):
        poly = [(-0.8, -0.6), (0.7, -0.7), (0.2, 0.1), (0.8, 0.7), (-0.6, 0.5)]
        pts = f32_points(poly[::-1] if rev else poly)
        parts = polyline_parts(pts, 0.2, off, clip, True, join, Cap.Butt, Cap.Butt)
        out.append(Case(f"join-closed-{join.name}-clip{clip}-off{off}-{'rev' if rev else 'fwd'}",
                        [stroke_case_shape(pts, 0.2, off, clip, True, DynamicStrokeOptions.Solid(join, Cap.Butt, Cap.Butt))],
                        place(size, size, size / 2, size / 2, 80.0, **TRANSFORMS["sheared" if rev else "rotated"]), size, size, msaa=4 if rev else 1,
                        model=parts_model(parts, 2 * 80.0, 40, hull=polyline_hull_points(pts, 0.2, off, clip, True))))
    return out


# ---- B. caps

def cap_cases():
    out = []
    size, scale, w = 160, 60.0, 0.5
    kinds = list(Cap)
    for i, start in enumerate(kinds):
        end = kinds[(i + 3) % len(kinds)]
        offset = (0.0, 0.3, -0.5, 0.2, 0.0, -0.25, 0.5)[i]
        pts = f32_points([(-0.9, -0.4), (0.8, 0.5)])
        tname = list(TRANSFORMS)[i % 4]
        parts = polyline_parts(pts, w, offset, 4.0, False, Join.Miter, start, end)
        out.append(Case(f"cap-{start.name}-{end.name}-off{offset}-{tname}",
                        [stroke_case_shape(pts, w, offset, 4.0, False, DynamicStrokeOptions.Solid(Join.Miter, start, end))],
                        place(size, size, size / 2 + 0.4, size / 2 - 0.3, scale, **TRANSFORMS[tname]), size, size, msaa=(1, 4)[i % 2],
                        model=parts_model(parts, 3 * scale, 30, hull=polyline_hull_points(pts, w, offset, 4.0, False))))
    return out


# ---- C. dashes

def dash_cases():
    out = []
    size = 256
    caps = list(Cap)
    patterns = [
        ([(1.0, 2.0)], 0.75),
        ([(0.5, 1.5), (2.5, 3.0)], -1.3),
        ([(0.7, 1.4), (2.0, 2.6), (3.5, 4.5)], 9.1),
        ([(0.4, 0.9), (1.3, 1.6), (2.2, 2.9), (3.3, 3.6)], -7.25),
    ]
    for i, (intervals, phase) in enumerate(patterns):
        pattern = [DashInterval(a, b, caps[(i + k) % 7], caps[(i + 2 * k + 3) % 7]) for k, (a, b) in enumerate(intervals)]
        w = 0.09
        pts = f32_points([(-0.9, -0.2), (0.9, 0.3)])
        parts = polyline_parts(pts, w, (0.0, 0.25)[i % 2], 4.0, False, Join.Miter, None, None, dash=(pattern, phase))
        out.append(Case(f"dash-{len(pattern)}-intervals-phase{phase}",
                        [stroke_case_shape(pts, w, (0.0, 0.25)[i % 2], 4.0, False, DynamicStrokeOptions.Dashed(Join.Miter, pattern, phase))],
                        place(size, size, size / 2, size / 2, 120.0, **TRANSFORMS[list(TRANSFORMS)[i]]), size, size, msaa=(1, 4)[i % 2],
                        model=parts_model(parts, 240.0, 40, hull=polyline_hull_points(pts, w, (0.0, 0.25)[i % 2], 4.0, False))))
    # the coordinate across joins: Butt dash caps, a pattern shorter than a join's arc so that dashes start and end inside wedges
    for join, clip in ((Join.Miter, 4.0), (Join.Round, 4.0)):
        pattern = [DashInterval(0.3, 0.55, Cap.Butt, Cap.Butt), DashInterval(0.8, 1.0, Cap.Butt, Cap.Butt)]
        pts = f32_points([(-0.8, -0.6), (-0.1, -0.45), (-0.3, 0.5), (0.7, 0.1), (0.2, -0.7)])
        w = 0.5
        parts = polyline_parts(pts, w, 0.0, clip, False, join, None, None, dash=(pattern, 0.1))
        out.append(Case(f"dash-across-{join.name}-joins", [stroke_case_shape(pts, w, 0.0, clip, False, DynamicStrokeOptions.Dashed(join, pattern, 0.1))],
                        place(size, size, size / 2, size / 2, 100.0), size, size, model=parts_model(parts, 200.0, 40, hull=polyline_hull_points(pts, w, 0.0, clip, False))))
    # a long path: 2400 segments, more than 5 000 widths, the length sums in f32 one after the other (k_stroke_lengths)
    rng = np.random.RandomState(11)
    n, w = 2400, 0.003
    angle = np.cumsum(rng.uniform(-0.5, 0.5, n) + 0.9 * np.where(np.arange(n) % 60 < 30, 1, -1) * 0.05)
    steps = np.stack([np.cos(angle), np.sin(angle)], axis=1) * 0.0095
    raw = np.cumsum(np.vstack([[0.0, 0.0], steps]), axis=0)
    raw = (raw - raw.min(axis=0)) / (raw.max(axis=0) - raw.min(axis=0)).max() * 1.8 - 0.9
    pts = f32_points(raw)
    length = sum(np.linalg.norm(np.subtract(b, a)) for a, b in zip(pts[:-1], pts[1:])) / w
    assert length >= 5000, length
    pattern = [DashInterval(3.0, 6.0, Cap.Butt, Cap.Butt)]
    size = 1024
    px_per_width = w * size * 0.5
    # the serial f32 sum of n terms of a total s is off by at most n * 2^-24 * s (widths), plus one f32 acos per join; across the stroke the
    # usual eps holds. Distances along the path are weighted by eps / (eps + drift) so that one eps test demands both.
    eps = f32_eps(size, size, size)
    drift = (n * G.F32_ULP * length + 2 * n * G.F32_ULP) * px_per_width
    parts = polyline_parts(pts, w, 0.0, 4.0, False, Join.Round, None, None, dash=(pattern, 0.0, eps / (eps + drift)))
    out.append(Case("dash-long-path", [stroke_case_shape(pts, w, 0.0, 4.0, False, DynamicStrokeOptions.Dashed(Join.Round, pattern, 0.0))],
                    place(size, size, size / 2, size / 2, size * 0.5), size, size, model=parts_model(parts, size, 200, eps=eps, hull=polyline_hull_points(pts, w, 0.0, 4.0, False))))
    return out


# ---- D. curved strokes

def curve_cases():
    """UniformlySpacedParameters(n): the stroke is the strip through P(t_i) +- the exact normal at t_i = i / n (stroke.rs:30-50, curve.rs),
    offset along it; the quads between consecutive parameters are the region."""
    out = []
    size, scale, w = 256, 100.0, 0.14
    specs = [
        (SegmentType.IntegralQuadraticCurve, lambda p: p.push_integral_quadratic_curve((0.0, 1.2), (0.8, -0.3)), 24),
        (SegmentType.IntegralCubicCurve, lambda p: p.push_integral_cubic_curve((-0.3, 1.1), (0.4, -1.1), (0.9, 0.4)), 40),
        (SegmentType.RationalQuadraticCurve, lambda p: p.push_rational_quadratic_curve(3.0, (0.0, 0.9), (0.8, -0.3)), 48),
        (SegmentType.RationalCubicCurve, lambda p: p.push_rational_cubic_curve((1.0, 0.4, 2.5, 1.0), (-0.3, 1.1), (0.4, -1.1), (0.9, 0.4)), 48),
    ]
    for i, (kind, push, steps) in enumerate(specs):
        offset = (0.0, 0.3, -0.4, 0.2)[i]
        path = Path(start=(-0.8, -0.3))
        push(path)
        path.stroke_options = StrokeOptions(w, offset, 4.0, False, 0, CurveApproximation.UniformlySpacedParameters(steps))
        tt = np.arange(steps + 1) / steps
        pts = G.bezier_points(path.start, kind, path.records[0], tt)
        h = 1e-6
        tan = np.array([unit(d) for d in (G.bezier_points(path.start, kind, path.records[0], np.clip(tt + h, 0, 1))
                                          - G.bezier_points(path.start, kind, path.records[0], np.clip(tt - h, 0, 1)))])
        nrm = np.stack([tan[:, 1], -tan[:, 0]], axis=1)
        lo, hi = pts + nrm * (offset - 0.5) * w, pts + nrm * (offset + 0.5) * w
        parts = []
        for k in range(steps):
            quad = [lo[k], hi[k], hi[k + 1], lo[k + 1]]
            assert G.is_convex(quad)
            parts.append((quad, (lambda quad: lambda p: G.convex_polygon(p, quad))(quad)))
        # the proto-hull: every strip vertex, the cap quads' outer corners half a width beyond both ends included (stroke.rs:270-282,444-462)
        caps = [pts[0] - tan[0] * 0.5 * w, pts[-1] + tan[-1] * 0.5 * w]
        hull = list(lo) + list(hi) + [q + nv * lat * w for q, nv in zip(caps, (nrm[0], nrm[-1])) for lat in (offset - 0.5, offset + 0.5)]
        out.append(Case(f"curve-{kind.name}-n{steps}-off{offset}", [([DynamicStrokeOptions.Solid(Join.Miter, Cap.Butt, Cap.Butt)], [path])],
                        place(size, size, size / 2, size / 2, scale, **TRANSFORMS[list(TRANSFORMS)[i]]), size, size, msaa=(1, 4)[i % 2],
                        model=parts_model(parts, 2 * scale, 60, hull=hull)))
    return out


# ---- E. fills and the winding rule

def fill_model(paths_of_shapes, flatten_samples=256, min_near=60):
    """Coverage: the winding number of every sample with respect to the exact curves (flattened in float64), non-zero modulo
    2^winding_bits (renderer.rs:397-402); eps = the f32 bound + the flattening's chord error."""
    def model(case):
        polys, err = [], 0.0
        for s, paths in enumerate(paths_of_shapes):
            for path in paths:
                polys.append(G.to_pixels(G.flatten(path, flatten_samples), case.transforms[s], case.width, case.height))
                err = max(err, G.flatten_error(path, flatten_samples, case.transforms[s], case.width, case.height))
        wn = G.winding_grid(polys, case.width, case.height, case.msaa)
        inside = np.mod(wn, 1 << case.winding_bits) != 0
        extent = max(float(np.abs(p).max()) for p in polys)
        eps = f32_eps(case.width, case.height, extent) + err
        near = G.near_distance(polys, case.width, case.height, case.msaa, 0.5)
        sd = np.where(np.isfinite(near), near, 1.0)
        return inside, sd, eps, min_near
    return model


def reversed_path(path):
    """A reversed copy (Path.reverse works in place, path.rs:445-488)."""
    import copy
    out = copy.deepcopy(path)
    out.reverse()
    return out


def nested_squares(windings):
    """Concentric squares; ring k (from outside) ends up with winding number windings[k]: each step's difference is that many copies of
    the square, clockwise (y up) for a positive step, reversed for a negative one."""
    paths, prev = [], 0
    for k, wn in enumerate(windings):
        half = 0.95 - k * 0.9 / len(windings)
        base = Path.from_rect((0.0, 0.0), (half, half * 0.8))
        step = wn - prev
        for _ in range(abs(step)):
            paths.append(base if step > 0 else reversed_path(base))
        prev = wn
    return paths


def fill_cases():
    out = []
    size = 200
    # rational quadratics and cubics, weights 0.2 - 5, integral quadratics, a loop and a cusp; clockwise in y up (the cubic fill is exact for
    # that orientation only, LAB_NOTEBOOK.md "Orientation convention of cubic fills"; quadratics for both)
    shapes = []
    p = Path(start=(-0.8, -0.6))
    p.push_rational_quadratic_curve(5.0, (-0.9, 0.7), (0.1, 0.6))
    p.push_rational_quadratic_curve(0.2, (0.9, 0.8), (0.7, -0.5))
    p.push_integral_quadratic_curve((0.0, -0.1), (-0.8, -0.6))
    shapes.append(p)
    q = Path(start=(-0.7, -0.7))
    q.push_rational_cubic_curve((1.0, 4.0, 0.3, 1.0), (-0.8, 0.8), (0.2, 0.9), (0.6, 0.4))
    q.push_rational_cubic_curve((1.0, 0.25, 2.0, 1.0), (0.9, 0.1), (0.6, -0.9), (-0.7, -0.7))
    shapes.append(q)
    loop = Path(start=(-0.6, -0.5))
    loop.push_integral_cubic_curve((1.4, 1.2), (-1.4, 1.2), (0.6, -0.5))
    loop.push_line((-0.6, -0.5))
    shapes.append(loop)
    cusp = Path(start=(-0.7, -0.6))
    cusp.push_integral_cubic_curve((0.9, 0.9), (-0.9, 0.9), (0.7, -0.6))
    cusp.push_line((-0.7, -0.6))
    shapes.append(cusp)
    for i, path in enumerate(shapes):
        for j, tname in enumerate(("identity", "mirrored") if i < 2 else ("sheared",)):
            out.append(Case(f"fill-curves{i}-{tname}-msaa{(1, 4)[j]}", [([], [path])], place(size, size, size / 2 + 0.3, size / 2 - 0.2, 88.0, **TRANSFORMS[tname]),
                            size, size, msaa=(1, 4)[j], model=fill_model([[path]]), fills_only=True))
    # the winding rule: rings of winding numbers around the wrap points of each counter width, both signs
    for bits, rings in ((1, [1, 2, 3, -1, -2]), (2, [3, 4, 5, -4, -3, 1]), (4, [15, 16, 17, -16, -15, 20]), (8, [255, 256, 257, -1, 0, 3])):
        paths = nested_squares(rings)
        out.append(Case(f"fill-winding-bits{bits}", [([], paths)], place(size, size, size / 2, size / 2, 96.0, **TRANSFORMS["rotated"]), size, size,
                        winding_bits=bits, model=fill_model([paths], 4), fills_only=True))
    # large frames: 2048 x 1536 and an 8192 x 48 strip, coordinates to 8192 (where f32 edge arithmetic has the fewest bits to spare)
    circle = Path.from_circle((0.0, 0.0), 1.0)
    ring = [Path.from_circle((0.0, 0.0), 1.0), reversed_path(Path.from_circle((0.0, 0.0), 0.6))]
    out.append(Case("fill-frame-2048x1536", [([], ring), ([], [circle])],
                    [place(2048, 1536, 1200.3, 700.7, 690.0), place(2048, 1536, 400.2, 300.9, 260.0, shear=0.3)], 2048, 1536,
                    model=fill_model([ring, [circle]], 2048, 200), fills_only=True))
    strip = [Path.from_rect((0.0, 0.0), (1.0, 1.0))]
    out.append(Case("fill-strip-8192x48", [([], ring), ([], strip)],
                    [place(8192, 48, 8100.4, 24.3, 20.0), place(8192, 48, 4096.0, 24.0, 4080.25, rotate=0.002)], 8192, 48, msaa=4,
                    model=fill_model([ring, strip], 512, 200), fills_only=True))
    return out


# ---- F. colour

def premultiplied_over(layers, n_samples_shape):
    """Per-sample float64 'over' of premultiplied covers (shaders.wgsl:305-309, the fixed blend One / OneMinusSrcAlpha): layers =
    [(coverage [P, S] bool, rgba non-premultiplied)] in draw order -> [P, S, 4]."""
    dst = np.zeros(n_samples_shape + (4,))
    for cov, c in layers:
        src = np.array([c[0] * c[3], c[1] * c[3], c[2] * c[3], c[3]], dtype=np.float64)
        dst = np.where(cov[..., None], src + dst * (1.0 - src[3]), dst)
    return dst


def colour_cases():
    out = []
    rng = np.random.RandomState(5)
    size = 128
    shapes, colors, regions, ts = [], [], [], []
    for k in range(28):
        cx, cy = rng.uniform(20, 108, 2)
        if k % 2:
            hx, hy = rng.uniform(8, 40, 2)
            shapes.append(([], [Path.from_rect((0.0, 0.0), (1.0, hy / hx))]))
            r = (lambda a: lambda p: G.convex_polygon(p, [(-1, -a), (-1, a), (1, a), (1, -a)]))(float(np.float32(hy / hx)))
            scale = hx
        else:
            scale = rng.uniform(6, 36)
            shapes.append(([], [Path.from_circle((0.0, 0.0), 1.0)]))
            r = lambda p: G.disc(p, (0.0, 0.0), 1.0)
        ts.append(place(size, size, cx, cy, scale, rotate=rng.uniform(0, 1)))
        colors.append([rng.uniform(0, 1), rng.uniform(0, 1), rng.uniform(0, 1), rng.uniform(0.15, 0.85)])
        regions.append(r)
    colors = np.float32(colors)

    def model(case, quantise=False):
        pix = G.samples(case.width, case.height, case.msaa).reshape(-1, 2)
        near = np.zeros(len(pix), dtype=bool)
        dst = np.zeros((len(pix), 4))
        eps = 0.0
        for s, region in enumerate(regions):
            t = case.transforms[s]
            sd = region(G.to_path(pix, t, case.width, case.height)) * G.min_pixel_scale(t, case.width, case.height)
            e = f32_eps(case.width, case.height, 2 * 40.0)  # (the discs are modelled as exact circles: Path.from_circle is rational, exact)
            eps = max(eps, e)
            near |= np.abs(sd) <= e
            c = np.float64(case.colors[s])
            src = np.array([c[0] * c[3], c[1] * c[3], c[2] * c[3], c[3]])
            dst = np.where((sd > 0)[:, None], src + dst * (1.0 - src[3]), dst)
            if quantise:  # an Rgba8Unorm attachment: every blend's result is stored as unorm8 (round to nearest)
                dst = np.where((sd > 0)[:, None], np.floor(dst * 255.0 + 0.5) / 255.0, dst)
        dst = dst.reshape(case.height * case.width, case.msaa, 4).mean(axis=1)
        ok = ~near.reshape(-1, case.msaa).any(axis=1)
        return dst.reshape(case.height, case.width, 4), ok.reshape(case.height, case.width)

    t = np.stack(ts)
    # RGBA8: the frame blends in f32 and rounds the resolved value to the nearest unorm8 once, half a unit; f32 adds at most 28 blends, the
    # premultiply and the 4-sample average, each one rounding of a value <= 1: 32 x 2^-24
    out.append(Case("colour-over-rgba8-msaa4", shapes, t, size, size, msaa=4, colors=colors, kind="colour", fills_only=True,
                    model=lambda case: model(case) + (0.5 / 255.0 + 32 * G.F32_ULP,)))
    out.append(Case("colour-over-rgba8-attachment", shapes, t, size, size, colors=colors, kind="colour", fills_only=True, fmt=2,
                    # each blend rounds to unorm8 in the model and on the device alike; an f32 value within 32 x 2^-24 of a rounding boundary
                    # may round the other way, one unit, and a one-unit difference of dst shrinks by (1 - a) < 1 in every later blend, so the
                    # stored values differ by at most one unit
                    model=lambda case: model(case, quantise=True) + (1.0 / 255.0 + 32 * G.F32_ULP,)))
    out.append(Case("colour-over-rgba16f", shapes, t, size, size, colors=colors, kind="colour", fills_only=True, fmt=1,
                    # binary16: at most 28 blends each rounded to 11 bits (2^-11 relative of a value <= 1), + the final conversion
                    model=lambda case: model(case) + ((28 + 1) * 2.0 ** -11,)))
    return out


CASES = join_cases() + cap_cases() + dash_cases() + curve_cases() + fill_cases() + colour_cases()


# ---------------------------------------------------------------- backends

GPU_PATHS = {
    "default": [],
    "triangles": [("CRH_TRIANGLE_PASS", "1")],
    "edges": [("CRH_EDGE_PASS", "1"), ("CRH_FILL_KERNEL", "0")],
    "rows": [("CRH_ROWS", "1")],
    "ops": [],  # the general kernel: the frame keeps its pass state (crh_frame_keep_pass_state), which only the general kernel serves
}


def path_ran(path, msaa, fills_only, t):
    """Did the pass t (test_gpu_fuzz.last_pass) run the raster path `path`?"""
    if path == "ops":
        return t["general"] == 1 and t["raster"] == "ops"
    if t["general"] != 0:
        return False
    if path == "triangles":
        return t["formulation"] == 2 and t["raster"] == "tile"
    if path == "rows":
        return t["formulation"] == 3 and t["raster"] in ("rows", "rows-long")
    if path == "edges":
        return t["formulation"] == 1 and t["raster"] in ("edges", "edges-long")
    # the default: the edge formulation on a plain kernel — k_raster_fill for fill-only msaa-1 passes (as border_path_ran in
    # test_gpu_fuzz.py), the per-sample edge kernel for strokes and at msaa 4
    if fills_only and msaa == 1:
        return t["formulation"] == 1 and t["raster"] == "fill"
    return t["formulation"] == 1 and t["raster"] in ("edges", "edges-long")


def render_oracle(case):
    from oracle.binding import Oracle
    o = Oracle(case.batch)
    assert o.status() == 0, o.status()
    return [o.render(case.width, case.height, case.msaa, case.winding_bits, case.transforms, case.colors, attachment8=case.fmt == 2)]


def render_gpu(case, path, monkeypatch):
    import torch
    assert torch.cuda.is_available()
    from contrast_renderer_amd import renderer as R
    from test_gpu_fuzz import _no_path_pins, last_pass
    _no_path_pins(monkeypatch)
    for name, value in GPU_PATHS[path]:
        monkeypatch.setenv(name, value)
    r = R.Renderer(R.Configuration(msaa_sample_count=case.msaa, clip_nesting_counter_bits=0, winding_counter_bits=case.winding_bits), device=0)
    scene = R.Scene(r, case.batch)
    assert scene.status() == 0
    frame = R.Frame(r, case.width, case.height, format=case.fmt)
    images = []
    for k in range(2):  # the verified pass, then the pass with the lists in place
        frame.clear()
        if path == "ops":
            frame.keep_pass_state()
        scene.render(frame, case.transforms, case.colors)
        images.append(frame.download())
        t = last_pass(frame)
        assert path_ran(path, case.msaa, case.fills_only, t), (case.name, path, k, t)
    return images


def check(case, image):
    if case.kind == "colour":
        expect, ok, tol = case.model(case)
        got = image.astype(np.float64) / (1.0 if image.dtype == np.float16 else 255.0)
        diff = np.abs(got - expect).max(axis=2)
        bad = ok & (diff > tol)
        assert not bad.any(), f"{case.name}: {int(bad.sum())} pixels off by more than {tol:.2e} (worst {diff[ok].max():.4f})"
        assert ok.sum() > 0.5 * ok.size and (expect[..., 3][ok] > 0).sum() > 2000
        return
    inside, sd, eps, min_near = case.model(case)
    covered = np.rint(image[..., 3].reshape(-1).astype(np.float64) / 255.0 * case.msaa).astype(int)
    G.check_coverage(covered, inside, sd, eps, min_near, case.name)


IDS = [c.name for c in CASES]


def test_the_cases_cover_every_family():
    names = " ".join(IDS)
    for family in ("join-Miter", "join-Bevel", "join-Round", "reversal", "collinear", "join-closed", "cap-", "dash-", "dash-across", "dash-long",
                   "curve-", "fill-curves", "fill-winding-bits8", "fill-frame", "fill-strip", "colour-over"):
        assert family in names, family
    assert {c.msaa for c in CASES} == {1, 4}
    for kind in Cap:
        assert any(f"cap-{kind.name}-" in n for n in IDS) and any(f"-{kind.name}-off" in n for n in IDS), kind


# the oracle renders RGBA8 (and the RGBA8 attachment) only: the RGBA16F case runs on the device backends alone
ORACLE_CASES = [c for c in CASES if c.fmt != 1]


@pytest.mark.parametrize("case", ORACLE_CASES, ids=[c.name for c in ORACLE_CASES])
def test_oracle_matches_the_model(case, oracle_lib):
    for image in render_oracle(case):
        check(case, image)


GPU_RUNS = [(c, p) for c in CASES for p in GPU_PATHS if p != "rows" or (c.fills_only and c.msaa == 1)]


@pytest.mark.gpu
@pytest.mark.parametrize("case,path", GPU_RUNS, ids=[f"{c.name}-{p}" for c, p in GPU_RUNS])
def test_gpu_matches_the_model(case, path, monkeypatch):
    for image in render_gpu(case, path, monkeypatch):
        check(case, image)
