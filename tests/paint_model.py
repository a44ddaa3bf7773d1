"""The float64 model of gradient paints (include/contrast_hip.h, crh_scene_set_paints) and the scenes the paint tests draw: plain numpy, shared by
tests/test_paints_cpu.py (which runs the model alone) and tests/test_gpu_paints.py (which holds the device against it)."""
import numpy as np

from contrast_renderer_amd import renderer as R
from contrast_renderer_amd.renderer import BlendFactor as F
from contrast_renderer_amd.renderer import BlendOperation as O

import ground_truth_util as G
from test_ground_truth import f32_eps

# the standard sample locations of msaa 2 and 8 (include/contrast_hip.h), beside the two ground_truth_util knows
for _n, _p in ((2, [(12, 12), (4, 4)]), (8, [(9, 5), (7, 11), (13, 9), (5, 3), (3, 13), (1, 7), (11, 15), (15, 1)])):
    G.SAMPLE_OFFSETS.setdefault(_n, np.array(_p, dtype=np.float64) / 16.0)

ROUNDINGS_OF_T = 32


def t_error(extent_px, length_px):
    """Bound on the f32 error of the gradient parameter t, from the roundings of the documented evaluation. With E = the frame extent in pixels
    (every intermediate of the homography is at most E pixels, in path units E / s for a scale of s pixels per unit), L = the gradient length in
    pixels and u = 2^-24:
      the inverse homography's nine coefficients are stored as f32 (u each, three per row) and each row is two fmas (u each) over terms that
      sum to at most 3 E / s: (3 + 2) * 3 = 15 u E / s per coordinate, 15 sqrt(2) < 22 u E / s for the point; a projective instance divides
      (1 u more, relative); p - p0 rounds once per coordinate (2 u E / s); the dot product (a product and an fma) or the sum of squares and its square
      root round twice more on values of at most 2 E L / s^2 resp. 2 E / s, and the division by dot(d, d) resp. the radius once: 3 u.
    What the host rounds when it builds the table is not counted here because the model takes the same values: p0, p1, offsets and colours
    are the f32 fields of crh_paint, and d = p1 - p0 and dot(d, d) are evaluated once in f32, as include/contrast_hip.h says (raw_t below).
    A point error e moves t by e s / L, so all of it is at most (22 + 1 + 2 + 3 + 3) u E / L = 31 u E / L; the spread adds one rounding of t
    itself (|t| <= E / L): ROUNDINGS_OF_T = 32."""
    return ROUNDINGS_OF_T * G.F32_ULP * extent_px / length_px


def spread_t(t, spread):
    if spread == R.Spread.Repeat:
        return t - np.floor(t)
    if spread == R.Spread.Reflect:
        u = t - 2.0 * np.floor(t / 2.0)
        return np.where(u <= 1.0, u, 2.0 - u)
    return np.clip(np.where(np.isnan(t), 0.0, t), 0.0, 1.0)  # PAD's clamp takes NaN as 0 (include/contrast_hip.h, `non-finite`)


def raw_t(paint, p):
    """t at path positions p [N, 2], in float64, from the table's f32 values: p0 and p1 as crh_paint holds them, d = p1 - p0 and dot(d, d)
    evaluated once in f32 (include/contrast_hip.h)."""
    p0, p1 = np.float32(paint.p0), np.float32(paint.p1)
    if paint.kind == R.PaintKind.Linear:
        d = p1 - p0
        dd = np.float32(np.float32(d[0] * d[0]) + np.float32(d[1] * d[1]))
        return ((p - np.float64(p0)) @ np.float64(d)) / np.float64(dd)
    return np.hypot(*(p - np.float64(p0)).T) / np.float64(p1[0])


def stop_colour(paint, t):
    """-> [N, 4] straight RGBA at spread parameters t."""
    offs = [np.float64(np.float32(s.offset)) for s in paint.stops]
    cols = [np.float64(np.float32(s.color)) for s in paint.stops]
    out = np.tile(cols[0], (len(t), 1))
    for i in range(len(offs)):
        here = t >= offs[i]
        if i + 1 < len(offs) and offs[i + 1] > offs[i]:
            f = ((t - offs[i]) / (offs[i + 1] - offs[i]))[:, None]
            value = cols[i] + f * (cols[i + 1] - cols[i])
        else:
            value = np.tile(cols[i], (len(t), 1))
        out = np.where(here[:, None], value, out)
    return out


def max_slope(paint):
    """The largest change of a stop colour channel per unit t."""
    worst = 0.0
    for a, b in zip(paint.stops[:-1], paint.stops[1:]):
        if b.offset > a.offset:
            worst = max(worst, float(np.abs(np.float64(b.color) - np.float64(a.color)).max() / (np.float64(np.float32(b.offset)) - np.float64(np.float32(a.offset)))))
    return worst


def length_px(paint, transform, size):
    """The length in pixels of one unit of t, at least (the smallest singular value of path -> pixels)."""
    unit = float(np.hypot(*(np.float64(np.float32(paint.p1)) - np.float64(np.float32(paint.p0))))) if paint.kind == R.PaintKind.Linear else float(paint.p1[0])
    return unit * G.min_pixel_scale(transform, size, size)


def paint_source(paint, tint, p, eps_t):
    """-> (src [N, 4] premultiplied and clamped, near [N]): near = within eps_t of a hard stop or of a REPEAT seam (an integer t)."""
    t = raw_t(paint, p)
    near = np.zeros(len(t), dtype=bool)
    if paint.spread == R.Spread.Repeat:
        near |= np.abs(t - np.round(t)) <= eps_t
    t = spread_t(t, paint.spread)
    for a, b in zip(paint.stops[:-1], paint.stops[1:]):
        if b.offset == a.offset and tuple(a.color) != tuple(b.color):
            near |= np.abs(t - np.float64(np.float32(a.offset))) <= eps_t
    c = stop_colour(paint, t) * np.float64(np.float32(tint))[None, :]
    src = np.concatenate([c[:, :3] * c[:, 3:4], c[:, 3:4]], axis=1)
    return np.clip(np.nan_to_num(src, nan=0.0), 0.0, 1.0), near


def blend_src(dst, cover, src, s, attachment):
    """tests/test_gpu_blending.py blend() with a source per sample: dst, src [N, 4] float64, cover [N] bool."""
    k = np.clip(np.float64(s.constant), 0.0, 1.0)
    out = dst.copy()
    for ch in range(4):
        comp = (s.blend.alpha if ch == 3 else s.blend.color) if s.blend else None
        d, da, sc, sa = dst[:, ch], dst[:, 3], src[:, ch], src[:, 3]

        def factor(f):
            return {F.Zero: 0.0, F.One: 1.0, F.Src: sc, F.OneMinusSrc: 1.0 - sc, F.SrcAlpha: sa, F.OneMinusSrcAlpha: 1.0 - sa,
                    F.Dst: d, F.OneMinusDst: 1.0 - d, F.DstAlpha: da, F.OneMinusDstAlpha: 1.0 - da,
                    F.SrcAlphaSaturated: np.minimum(sa, 1.0 - da) if ch < 3 else 1.0, F.Constant: k[ch], F.OneMinusConstant: 1.0 - k[ch]}[F(f)]
        if comp is None:
            v = sc
        elif comp.operation == O.Min:
            v = np.minimum(sc, d)
        elif comp.operation == O.Max:
            v = np.maximum(sc, d)
        else:
            ps, qd = sc * factor(comp.src_factor), d * factor(comp.dst_factor)
            v = {O.Add: ps + qd, O.Subtract: ps - qd, O.ReverseSubtract: qd - ps}[O(comp.operation)]
        v = np.clip(v, 0.0, 1.0)
        if attachment:
            v = np.floor(v * 255.0 + 0.5) / 255.0
        if (int(s.write_mask) >> ch) & 1:
            out[:, ch] = np.where(cover, v, d)
    return out


def to_path_h(pix, m, size):
    """Pixel -> path coordinates through the float64 inverse of the instance's homography (any 4x4 transform)."""
    m = np.float64(m)
    cx, cy, cw = (np.array([m[r], m[4 + r], m[12 + r]]) for r in (0, 1, 3))
    H = np.stack([(cx * 0.5 + cw * 0.5) * size, (cw * 0.5 - cy * 0.5) * size, cw])
    q = (np.linalg.inv(H) @ np.concatenate([pix, np.ones((len(pix), 1))], axis=1).T).T
    return q[:, :2] / q[:, 2:3]


def model(size, msaa, transforms, colours, regions, paints, s, attachment, background):
    """Shapes drawn in order over `background` ([size, size, 4] linear float64 or RGBA8), shape i with paints[i] (None: its solid colour) ->
    (expected [H, W, 4] float64 linear, checkable [H, W], the largest (colour slope x t error) of the paints)."""
    pix = G.samples(size, size, msaa).reshape(-1, 2)
    bg = background.astype(np.float64) / 255.0 if background.dtype == np.uint8 else background
    dst = np.repeat(bg.reshape(-1, 4), msaa, axis=0)
    near = np.zeros(len(pix), dtype=bool)
    extra = 0.0
    for t, c, region, paint in zip(transforms, colours, regions, paints):
        p = G.to_path(pix, t, size, size)
        sd = region(p) * G.min_pixel_scale(t, size, size)
        near |= np.abs(sd) <= f32_eps(size, size, 2 * 40.0)
        if paint is None:
            tint = np.float64(np.float32(c))
            src = np.tile(np.clip([tint[0] * tint[3], tint[1] * tint[3], tint[2] * tint[3], tint[3]], 0.0, 1.0), (len(pix), 1))
        else:
            dt = t_error(size + 2 * 40.0, length_px(paint, t, size))
            extra = max(extra, max_slope(paint) * dt)
            src, seam = paint_source(paint, c, p, 4.0 * dt)
            near |= seam & (sd > -1.0)
        dst = blend_src(dst, sd > 0, src, s, attachment)
    expect = dst.reshape(size * size, msaa, 4).mean(axis=1).reshape(size, size, 4)
    return expect, ~near.reshape(-1, msaa).any(axis=1).reshape(size, size), extra


def random_stops(rng, n, hard=False, alpha=(0.3, 1.0)):
    offsets = np.linspace(0.0, 1.0, n) if n > 1 else np.array([0.5])
    if hard and n > 2:
        j = rng.randint(1, n - 1)
        offsets[j] = offsets[j - 1]
    return [R.GradientStop(float(np.float32(o)), tuple(float(np.float32(v)) for v in (*rng.uniform(0, 1, 3), rng.uniform(*alpha)))) for o in offsets]


def random_paint(rng, kind, spread, n_stops=None, hard=False):
    """A paint over a unit-sized shape: one unit of t is 1..2 path units long (the scenes scale a unit to at least 16 pixels)."""
    n = n_stops or rng.randint(2, 9)
    stops = random_stops(rng, n, hard)
    if kind == R.PaintKind.Linear:
        p0 = rng.uniform(-1.0, 0.0, 2)
        a, length = rng.uniform(0, 2 * np.pi), rng.uniform(1.0, 2.0)
        return R.Paint.linear(p0, p0 + length * np.array([np.cos(a), np.sin(a)]), stops, spread)
    return R.Paint.radial(rng.uniform(-0.5, 0.5, 2), rng.uniform(1.0, 1.5), stops, spread)


def scene(kind, spread, seed=5, size=128, n=12):
    """Twelve translucent discs and rectangles (tests/test_gpu_blending.py stack), every one with a paint of `kind` and `spread`, every other
    one with a hard stop -> (shapes, transforms, colours, regions, paints)."""
    from test_gpu_blending import stack
    shapes, transforms, colours, regions = stack(seed=seed, size=size, n=n, radius=(16, 36))
    rng = np.random.RandomState(seed + 100)
    paints = [random_paint(rng, kind, spread, hard=bool(i % 2)) for i in range(n)]
    return shapes, transforms, colours, regions, paints


def sweep_scene(size=128, n=20, seed=21):
    """Twenty discs and rectangles under random affine transforms — every third sheared, every fourth mirrored — with random paints (every
    seventh solid, every fifth with a hard stop) -> (shapes, transforms, colours, regions, paints)."""
    from contrast_renderer_amd import Path
    from test_ground_truth import place
    rng = np.random.RandomState(seed)
    shapes, transforms, colours, regions, paints = [], [], [], [], []
    kinds, spreads = (R.PaintKind.Linear, R.PaintKind.Radial), (R.Spread.Pad, R.Spread.Repeat, R.Spread.Reflect)
    for i in range(n):
        shear = rng.uniform(-0.5, 0.5) if i % 3 == 0 else 0.0
        t = place(size, size, *rng.uniform(24, size - 24, 2), rng.uniform(20, 34), rotate=rng.uniform(0, 6.28), mirror=i % 4 == 1, shear=shear)
        if i % 2:
            shapes.append(([], [Path.from_rect((0.0, 0.0), (1.0, 0.75))]))
            regions.append(lambda q: G.convex_polygon(q, [(-1, -0.75), (-1, 0.75), (1, 0.75), (1, -0.75)]))
        else:
            shapes.append(([], [Path.from_circle((0.0, 0.0), 1.0)]))
            regions.append(lambda q: G.disc(q, (0.0, 0.0), 1.0))
        transforms.append(t)
        colours.append([*rng.uniform(0.5, 1, 3), rng.uniform(0.3, 0.9)])
        paints.append(random_paint(rng, kinds[i % 2], spreads[rng.randint(3)], hard=i % 5 == 0) if i % 7 else None)
    return shapes, np.float32(np.stack(transforms)), np.float32(colours), regions, paints


def recorded_scene(size=128):
    """The recorded pass of the GPU test: a clip disc, two painted covers and a solid one inside it, under an opacity group ->
    (placements t_clip, t_all, transforms, colours, group colour, regions clipped by the disc, paints, the clip's signed distance in pixels per sample of msaa 4)."""
    from test_ground_truth import place
    rng = np.random.RandomState(4)
    grad_a, grad_b = random_paint(rng, R.PaintKind.Linear, R.Spread.Reflect, 4), random_paint(rng, R.PaintKind.Radial, R.Spread.Repeat, 3)
    t_clip, t_a, t_b = place(size, size, 64, 64, 44), place(size, size, 50, 60, 30, rotate=0.4), place(size, size, 80, 70, 26, rotate=-0.3)
    t_c, t_all = place(size, size, 64, 40, 20), place(size, size, 64, 64, 70)
    colours, group = [(1.0, 1.0, 1.0, 0.9), (0.9, 0.8, 1.0, 0.7), (0.2, 0.7, 0.4, 0.6)], (0.0, 0.0, 0.0, 0.5)
    unit_disc = lambda q: G.disc(q, (0.0, 0.0), 1.0)
    unit_rect = lambda q: G.convex_polygon(q, [(-1, -1), (-1, 1), (1, 1), (1, -1)])
    pix = G.samples(size, size, 4).reshape(-1, 2)
    clip_sd = unit_disc(G.to_path(pix, t_clip, size, size)) * G.min_pixel_scale(t_clip, size, size)

    def clipped(region, t):  # the shape's region intersected with the clip disc, in the shape's own units
        scale = G.min_pixel_scale(t, size, size)
        return lambda q: np.minimum(region(q) * scale, clip_sd) / scale
    regions = [clipped(unit_disc, t_a), clipped(unit_rect, t_b), clipped(unit_disc, t_c)]
    return t_clip, t_all, [t_a, t_b, t_c], colours, group, regions, [grad_a, grad_b, None], clip_sd


SCENES = [(kind, spread) for kind in (R.PaintKind.Linear, R.PaintKind.Radial) for spread in (R.Spread.Pad, R.Spread.Repeat, R.Spread.Reflect)]


def srgb_decode(code):
    """sRGB code (float64, may be fractional) / 255 -> linear."""
    x = np.asarray(code, dtype=np.float64) / 255.0
    return np.where(x <= 0.04045, x / 12.92, ((x + 0.055) / 1.055) ** 2.4)
