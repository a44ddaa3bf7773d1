"""The float64 model of conic gradient paints (include/contrast_hip.h, crh_scene_set_paints: CRH_PAINT_CONIC) and the scenes the conic tests draw:
plain numpy, shared by tests/test_conic_cpu.py (which runs the model alone) and tests/test_gpu_conic.py (which holds the device against it). The
spread, the stops, the blend and the shapes are paint_model's; this module adds the angle.

The table's values are taken as the header says the table holds them: s = (p1[0] / 2 pi) - floor(p1[0] / 2 pi) and k = 2 pi / |p1[1] - p1[0]|, each
evaluated in binary64 from the f32 fields and rounded once to f32. The angle itself is float64 atan2.

The f32 error of t at a sample rho pixels from the centre, for a sweep of w turns (k = 1 / w): a point error of e pixels turns the angle by
e / rho radians, which is e / (2 pi rho) turns and e / (2 pi rho w) of t — paint_model.t_error with the arc of one unit of t at that radius,
2 pi rho w pixels, as the gradient's length (it counts the roundings of the point, of p - p0 and three more). The device's angle is off by at most
the bound csrc/paint_angle.hpp states, kPaintTurnsError, read from the header here; a - s, the + 1 and the product with k round once each on values
below 1 resp. k, of which the first two count in turns (2 ulp) and the third is paint_model's rounding of t itself:
    t_error(extent, 2 pi rho w) + (kPaintTurnsError + 2 ulp) / w.
The error grows without bound towards the centre, and t jumps on the start ray, so the model leaves out the samples nearer than RHO_MIN = 3
pixels to a centre and those within four such errors of the start ray, of an integer t under REPEAT, or of a hard stop — besides the samples
on shape edges that paint_model leaves out."""
import math
import os
import re

import numpy as np

from contrast_renderer_amd import renderer as R
from contrast_renderer_amd.renderer import Spread

import ground_truth_util as G
import image_paint_model as IM
import paint_model as M
from test_ground_truth import f32_eps

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ANGLE_HEADER = os.path.join(ROOT, "contrast_renderer_amd", "csrc", "paint_angle.hpp")
RHO_MIN = 3.0
TURN = 2.0 * math.pi
TURN_F32 = float(np.float32(TURN))  # the f32 nearest to 2 pi: the largest |sweep|
SIZE = 128
OVER = R.ColorTargetState(R.BlendState.PREMULTIPLIED_ALPHA_BLENDING)


def angle_bound():
    """kPaintTurnsError of csrc/paint_angle.hpp, in turns."""
    return float(re.search(r"constexpr float kPaintTurnsError = ([0-9.eE+-]+)f;", open(ANGLE_HEADER).read()).group(1))


def is_conic(paint):
    return isinstance(paint, R.Paint) and int(paint.kind) == int(R.PaintKind.Conic)


def table(paint):
    """-> (s, k, direction) as the table holds them: float64 values of the f32 s and k, +1.0 or -1.0."""
    start, end = np.float64(np.float32(paint.p1[0])), np.float64(np.float32(paint.p1[1]))
    sweep = end - start
    s = np.float32(start / TURN - np.floor(start / TURN))
    k = np.float32(TURN / abs(sweep))
    return np.float64(s), np.float64(k), 1.0 if sweep > 0 else -1.0


def turns_fraction(paint):
    """w: the sweep in turns, as the table's k gives it."""
    return 1.0 / table(paint)[1]


def turns(dy, dx):
    a = np.arctan2(dy, dx) / TURN
    a = np.where(a < 0.0, a + 1.0, a)
    return np.where(a >= 1.0, 0.0, a)  # (-tiny / 2 pi + 1 rounds to 1 in float64 too: the same angle as 0)


def raw_b(paint, p):
    """b in [0, 1] at path positions p [N, 2]: the angle from the start ray in the sweep's direction, in turns."""
    s, _, direction = table(paint)
    p0 = np.float64(np.float32(paint.p0))
    a = turns(p[:, 1] - p0[1], p[:, 0] - p0[0])
    b = a - s if direction > 0 else s - a
    return np.where(b < 0.0, b + 1.0, b)


def raw_t(paint, p):
    return raw_b(paint, p) * table(paint)[1]


def t_of_one_sample(paint, x, y):
    """The header's definition, one sample at a time, with math alone: what raw_t is checked against."""
    cx, cy, start, end = (float(np.float32(v)) for v in (*paint.p0, *paint.p1))
    a = math.atan2(y - cy, x - cx) / TURN
    if a < 0.0:
        a += 1.0
    if a >= 1.0:
        a = 0.0
    sweep = end - start
    s = float(np.float32(start / TURN - math.floor(start / TURN)))
    k = float(np.float32(TURN / abs(sweep)))
    b = a - s if sweep > 0 else s - a
    if b < 0.0:
        b += 1.0
    return b * k


def t_error(paint, extent_px, rho_px):
    """The bound of the module's docstring at samples rho_px [N] pixels from the centre (at least RHO_MIN is taken)."""
    w = turns_fraction(paint)
    return M.t_error(extent_px, TURN * np.maximum(rho_px, RHO_MIN) * w) + (angle_bound() + 2.0 * G.F32_ULP) / w


def conic_source(paint, tint, p, dt, rho_px=None):
    """-> (src [N, 4] premultiplied and clamped, near [N]): near = nearer than RHO_MIN pixels to the centre (where rho_px is given), or within
    4 dt (a scalar or [N]) of the start ray, of an integer t under REPEAT, or of a hard stop."""
    _, k, _ = table(paint)
    b = raw_b(paint, p)
    t = b * k
    eps = 4.0 * np.broadcast_to(np.float64(dt), t.shape)
    near = (t <= eps) | ((1.0 - b) * k <= eps)
    if rho_px is not None:
        near |= rho_px < RHO_MIN
    if paint.spread == Spread.Repeat:
        near |= np.abs(t - np.round(t)) <= eps
    t = M.spread_t(t, paint.spread)
    for a, c in zip(paint.stops[:-1], paint.stops[1:]):
        if c.offset == a.offset and tuple(a.color) != tuple(c.color):
            near |= np.abs(t - np.float64(np.float32(a.offset))) <= eps
    col = M.stop_colour(paint, t) * np.float64(np.float32(tint))[None, :]
    src = np.concatenate([col[:, :3] * col[:, 3:4], col[:, 3:4]], axis=1)
    return np.clip(np.nan_to_num(src, nan=0.0), 0.0, 1.0), near


def model(size, msaa, transforms, colours, regions, paints, s, attachment, background):
    """paint_model.model with conic paints: paints[i] is None (the solid colour), a Paint of any kind or an image_paint_model.ImageSpec ->
    (expected [H, W, 4] float64 linear, checkable [H, W], the largest extra tolerance term of the paints, the share of the covered pixels
    that are not checkable)."""
    pix = G.samples(size, size, msaa).reshape(-1, 2)
    bg = background.astype(np.float64) / 255.0 if background.dtype == np.uint8 else background
    dst = np.repeat(bg.reshape(-1, 4), msaa, axis=0)
    near, covered = np.zeros(len(pix), dtype=bool), np.zeros(len(pix), dtype=bool)
    extent = size + 2 * 40.0
    extra = 0.0
    for t, c, region, paint in zip(transforms, colours, regions, paints):
        p = G.to_path(pix, t, size, size)
        scale = G.min_pixel_scale(t, size, size)
        sd = region(p) * scale
        near |= np.abs(sd) <= f32_eps(size, size, 2 * 40.0)
        covered |= sd > 0
        if paint is None:
            tint = np.float64(np.float32(c))
            src = np.tile(np.clip([tint[0] * tint[3], tint[1] * tint[3], tint[2] * tint[3], tint[3]], 0.0, 1.0), (len(pix), 1))
        elif isinstance(paint, IM.ImageSpec):
            u, v = IM.uv_of(paint, p[sd > -1.0])
            err = IM.uv_error(extent, IM.texel_px(paint, t, size), float(max(np.abs(u).max(), np.abs(v).max())) if len(u) else 0.0)
            extra = max(extra, IM.extra_of(paint, err))
            src, seam = IM.image_source(paint, c, p, err)
            near |= seam & (sd > -1.0)
        elif is_conic(paint):
            rho = np.hypot(*(p - np.float64(np.float32(paint.p0))).T) * scale
            dt = t_error(paint, extent, rho)
            extra = max(extra, M.max_slope(paint) * float(t_error(paint, extent, RHO_MIN)))
            src, seam = conic_source(paint, c, p, dt, rho)
            near |= seam & (sd > -1.0)
        else:
            dt = M.t_error(extent, M.length_px(paint, t, size))
            extra = max(extra, M.max_slope(paint) * dt)
            src, seam = M.paint_source(paint, c, p, 4.0 * dt)
            near |= seam & (sd > -1.0)
        dst = M.blend_src(dst, sd > 0, src, s, attachment)
    expect = dst.reshape(size * size, msaa, 4).mean(axis=1).reshape(size, size, 4)
    by_pixel = lambda a: a.reshape(-1, msaa).any(axis=1)
    left_out = (by_pixel(near) & by_pixel(covered)).sum() / max(1, by_pixel(covered).sum())
    return expect, ~by_pixel(near).reshape(size, size), extra, float(left_out)


# ---------------------------------------------------------------- paints and scenes

SWEEPS = {"turn": 1.0, "third": 1.0 / 3.0, "quarter": 0.25}
SPREADS = (Spread.Pad, Spread.Repeat, Spread.Reflect)
GRID = [(name, spread) for name in SWEEPS for spread in SPREADS]
MSAA_OF_GRID = {(name, spread): (1, 4) for name, spread in GRID}
MSAA_OF_GRID[("third", Spread.Repeat)] = (1, 2, 4)  # one case each of msaa 2 and 8 beside the grid's 1 and 4
MSAA_OF_GRID[("quarter", Spread.Reflect)] = (1, 4, 8)


def end_angle(start, sweep):
    """The f32 end angle of a sweep from the f32 `start`: start + sweep rounded to f32, one step back towards the start where the rounding
    carried |end - start| beyond the f32 nearest to 2 pi."""
    start = np.float32(start)
    end = np.float32(np.float64(start) + sweep)
    if abs(np.float64(end) - np.float64(start)) > TURN_F32:
        end = np.nextafter(end, start)
    assert 0.0 < abs(np.float64(end) - np.float64(start)) <= TURN_F32
    return float(end)


def random_conic(rng, fraction, spread, n_stops=None, hard=False, clockwise=False):
    """A conic paint over a unit-sized shape: the centre inside it, any start angle, a sweep of `fraction` turns (a full turn: the f32 nearest
    to 2 pi at the most)."""
    stops = M.random_stops(rng, n_stops or rng.randint(2, 9), hard)
    start = np.float32(rng.uniform(-7.0, 7.0))
    sweep = min(fraction * TURN, TURN_F32)
    return R.Paint.conic(rng.uniform(-0.5, 0.5, 2), float(start), end_angle(start, -sweep if clockwise else sweep), stops, spread)


def scene(sweep, spread, seed=5, size=SIZE, n=12):
    """paint_model.scene's twelve translucent discs and rectangles, every one with a conic paint of `spread` over SWEEPS[sweep] of a turn,
    every other one with a hard stop, every third one clockwise -> (shapes, transforms, colours, regions, paints)."""
    shapes, transforms, colours, regions, _ = M.scene(R.PaintKind.Linear, spread, seed=seed, size=size, n=n)
    rng = np.random.RandomState(seed + 500)
    paints = [random_conic(rng, SWEEPS[sweep], spread, hard=bool(i % 2), clockwise=i % 3 == 2) for i in range(n)]
    return shapes, transforms, colours, regions, paints


def sweep_scene(size=SIZE, n=20, seed=21):
    """paint_model.sweep_scene's twenty shapes under sheared and mirrored transforms with linear, radial and conic paints in turn (every
    seventh solid, every fifth with a hard stop), all three spreads."""
    shapes, transforms, colours, regions, paints = M.sweep_scene(size, n, seed)
    rng = np.random.RandomState(seed + 500)
    conics = 0
    for i in range(n):
        if paints[i] is not None and i % 3 == 2:
            paints[i] = random_conic(rng, (1.0, 1.0 / 3.0, 0.25)[rng.randint(3)], SPREADS[conics % 3], hard=i % 5 == 0, clockwise=bool(rng.randint(2)))
            conics += 1
    return shapes, transforms, colours, regions, paints


def mixed_scene(size=SIZE, seed=8):
    """Five shapes of the stack in one pass: a linear, a radial, a conic, an image-painted and a solid instance."""
    from test_gpu_blending import stack
    shapes, transforms, colours, regions = stack(seed=seed, size=size, n=5, radius=(20, 36))
    rng = np.random.RandomState(seed + 500)
    image = IM.placed(IM.random_image(rng, 8, 8), 0.3, 0.7, (7.0, 1.0), R.Filter.Linear, Spread.Reflect, Spread.Repeat)
    paints = [M.random_paint(rng, R.PaintKind.Linear, Spread.Reflect, 4), M.random_paint(rng, R.PaintKind.Radial, Spread.Repeat, 3),
              random_conic(rng, 1.0 / 3.0, Spread.Reflect, 5, hard=True), image, None]
    return shapes, transforms, colours, regions, paints


def quadrant_paint(start=0.0, clockwise=False, colours=None):
    """Four colours with hard stops at 0.25, 0.5 and 0.75 over a full turn round the origin."""
    c = colours or [(1.0, 0.0, 0.0, 1.0), (0.0, 1.0, 0.0, 1.0), (0.0, 0.0, 1.0, 1.0), (1.0, 1.0, 0.0, 1.0)]
    stops = [(0.0, c[0]), (0.25, c[0]), (0.25, c[1]), (0.5, c[1]), (0.5, c[2]), (0.75, c[2]), (0.75, c[3]), (1.0, c[3])]
    return R.Paint.conic((0.0, 0.0), float(np.float32(start)), end_angle(start, -TURN_F32 if clockwise else TURN_F32), stops, Spread.Pad)


def gpu_scenes():
    """(name, scene, sample counts) of every scene tests/test_gpu_conic.py holds against model()."""
    out = [(f"{name}-{spread.name}", scene(name, spread), MSAA_OF_GRID[(name, spread)]) for name, spread in GRID]
    out.append(("srgb", scene("third", Spread.Reflect, seed=9), (4,)))
    out.append(("blend-state", scene("quarter", Spread.Repeat, seed=6), (4,)))
    out.append(("mixed", mixed_scene(), (4,)))
    out.append(("sweep", sweep_scene(), (4,)))
    return out


# ---------------------------------------------------------------- the angle alone: csrc/paint_angle.hpp through its stand-alone program

def special_pairs():
    """(y, x) f32 pairs [N, 2]: the axes, the diagonals, every sign of zero, y = -tiny, at magnitudes from the smallest denormal to 2^24."""
    tiny = np.float32(2.0 ** -149)
    out = [(sy * 0.0, sx * 0.0) for sy in (1.0, -1.0) for sx in (1.0, -1.0)]
    for e in (-149, -140, -127, -126, -60, -1, 0, 1, 10, 23, 24):
        m = np.float32(2.0 ** e)
        out += [(0.0, m), (m, 0.0), (0.0, -m), (-m, 0.0), (-0.0, m), (-0.0, -m), (m, -0.0), (-m, -0.0)]
        out += [(m, m), (m, -m), (-m, -m), (-m, m), (-tiny, m), (-tiny, -m), (tiny, m), (m, tiny), (m, -tiny)]
    return np.array(out, dtype=np.float32)


def dense_pairs(per_turn=2048, exponents=range(-140, 25, 4)):
    """(y, x) f32 pairs [N, 2]: per_turn angles off the axes and diagonals in every octant, at each magnitude 2^e."""
    theta = TURN * (np.arange(per_turn) + 0.37) / per_turn
    unit = np.stack([np.sin(theta), np.cos(theta)], axis=1)
    return np.concatenate([np.float32(unit * 2.0 ** e) for e in exponents])


def random_pairs(n, seed=77):
    """(y, x) f32 pairs [N, 2] of random angle and magnitude 2^-140 .. 2^24."""
    rng = np.random.RandomState(seed)
    theta, m = rng.uniform(0.0, TURN, n), 2.0 ** rng.uniform(-140.0, 24.0, n)
    return np.float32(np.stack([np.sin(theta) * m, np.cos(theta) * m], axis=1))


def build_angle_program(directory):
    """Compiles tests/cpp/paint_angle_harness.cpp against csrc/paint_angle.hpp alone with the host compiler -> the program's path."""
    import subprocess
    out = os.path.join(directory, "paint_angle_harness")
    cmd = ["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror", "-I", os.path.dirname(ANGLE_HEADER),
           os.path.join(ROOT, "tests", "cpp", "paint_angle_harness.cpp"), "-o", out]
    done = subprocess.run(cmd, capture_output=True, text=True)
    assert done.returncode == 0, done.stderr
    return out


def host_turns(program, pairs, directory):
    """paint_turns(y, x) of the f32 pairs [N, 2], evaluated on the host by the stand-alone program -> f32 [N]."""
    import subprocess
    src, dst = os.path.join(directory, "pairs.f32"), os.path.join(directory, "turns.f32")
    np.ascontiguousarray(pairs, dtype=np.float32).tofile(src)
    done = subprocess.run([program, src, dst], capture_output=True, text=True)
    assert done.returncode == 0, (done.returncode, done.stderr)
    out = np.fromfile(dst, dtype=np.float32)
    assert out.shape == (len(pairs),)
    return out
