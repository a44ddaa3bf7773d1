"""The float64 model of image paints (include/contrast_hip.h, crh_scene_set_paints_with_images) and the scenes the image paint tests draw: plain
numpy, shared by tests/test_image_paints_cpu.py (which runs the model alone) and tests/test_gpu_image_paints.py (which holds the device against it).

The f32 error of (u, v), in texels, from the roundings of the documented evaluation. With E = the frame extent in pixels, s = the instance's
scale in pixels per path unit, tau = the size of a texel in pixels (the path -> texel map stretches a path distance d to d s / tau texels),
U = the largest |u| or |v| the shape reaches and ulp = 2^-24:
  the point p — paint_model.t_error derives it: the inverse homography's nine coefficients are stored as f32 and each row is two fmas over terms
  that sum to at most 3 E / s, (3 + 2) * 3 = 15 ulp E / s per coordinate, 15 sqrt(2) < 22 ulp E / s for the point, and a projective instance
  divides, one relative ulp more: 23 ulp E / s, which the map to texels stretches to 23 ulp E / tau;
  u = fma(p.y, m1, fma(p.x, m0, m2)) rounds twice on values of at most U (m is the f32 table the model reads too): 2 ulp U; the same for v;
  LINEAR subtracts 0.5, one rounding of a value of at most U + 1/2; floor is exact and a - floor(a) is exact (Sterbenz): 1 ulp U.
So each coordinate is off by at most uv_error = (23 E / tau + 3 U) ulp texels. A bilinear value moves by at most D per texel along each axis,
D = the largest channel difference between neighbouring texels of the wrapped image, so by at most 2 D uv_error for an error in both
coordinates: the term the tests add to the tolerance of the blending tests (the texel's own (float)k / 255.0f, the two lerps and the tint's
products are roundings of values <= 1, of the order the 512 ulp there cover). A NEAREST sample takes another texel only when (u, v) is within
the error of a texel boundary: a pixel with a sample whose value changes within 4 uv_error in any direction is not checked, as hard stops
are not in the gradient tests."""
from collections import namedtuple

import numpy as np

from contrast_renderer_amd import renderer as R
from contrast_renderer_amd.renderer import Filter, Spread

import ground_truth_util as G
import paint_model as M
from test_ground_truth import f32_eps

ImageSpec = namedtuple("ImageSpec", "pixels matrix filter spread_x spread_y")  # what an ImagePaint holds, with the texels on the host
ROUNDINGS_OF_P, ROUNDINGS_OF_UV = 23, 3
OVER = R.ColorTargetState(R.BlendState.PREMULTIPLIED_ALPHA_BLENDING)
SIZE = 128
SPREADS = [(Spread.Pad, Spread.Pad), (Spread.Repeat, Spread.Reflect), (Spread.Reflect, Spread.Repeat)]


def uv_error(extent_px, texel_px, uv_max):
    return (ROUNDINGS_OF_P * extent_px / texel_px + ROUNDINGS_OF_UV * uv_max) * G.F32_ULP


def wrap(i, n, spread):
    if spread == Spread.Repeat:
        return i - n * np.floor_divide(i, n)
    if spread == Spread.Reflect:
        k = i - 2 * n * np.floor_divide(i, 2 * n)
        return np.where(k < n, k, 2 * n - 1 - k)
    return np.clip(i, 0, n - 1)


def uv_of(spec, p):
    m = np.float64(np.float32(spec.matrix))
    u, v = m[0] * p[:, 0] + m[1] * p[:, 1] + m[2], m[3] * p[:, 0] + m[4] * p[:, 1] + m[5]
    limit = 2.0 ** 24
    return np.clip(np.nan_to_num(u, nan=0.0), -limit, limit), np.clip(np.nan_to_num(v, nan=0.0), -limit, limit)


def sample(spec, u, v):
    """-> [N, 4] premultiplied value of the image at texel coordinates (u, v), float64."""
    T = spec.pixels.astype(np.float64) / 255.0
    h, w = T.shape[:2]
    if spec.filter == Filter.Nearest:
        return T[wrap(np.floor(v).astype(np.int64), h, spec.spread_y), wrap(np.floor(u).astype(np.int64), w, spec.spread_x)]
    a, b = u - 0.5, v - 0.5
    i, j = np.floor(a).astype(np.int64), np.floor(b).astype(np.int64)
    fx, fy = (a - i)[:, None], (b - j)[:, None]
    i0, i1, j0, j1 = wrap(i, w, spec.spread_x), wrap(i + 1, w, spec.spread_x), wrap(j, h, spec.spread_y), wrap(j + 1, h, spec.spread_y)
    top = T[j0, i0] + fx * (T[j0, i1] - T[j0, i0])
    bottom = T[j1, i0] + fx * (T[j1, i1] - T[j1, i0])
    return top + fy * (bottom - top)


def neighbour_difference(spec):
    """The largest channel difference between neighbouring texels of the wrapped image (REPEAT: the last and the first are neighbours; under PAD
    and REFLECT a border texel's neighbour is itself)."""
    T = spec.pixels.astype(np.float64) / 255.0
    worst = 0.0
    for axis, spread in ((1, spec.spread_x), (0, spec.spread_y)):
        if T.shape[axis] > 1:
            worst = max(worst, float(np.abs(np.diff(T, axis=axis)).max()))
            if spread == Spread.Repeat:
                worst = max(worst, float(np.abs(np.take(T, 0, axis=axis) - np.take(T, -1, axis=axis)).max()))
    return worst


def texel_px(spec, transform, size):
    """The size of a texel in pixels, at least: 1 / the largest singular value of pixels -> texels."""
    m = np.float64(np.float32(spec.matrix))
    to_texels = np.array([[m[0], m[1]], [m[3], m[4]]]) @ np.linalg.inv(G.pixel_jacobian(transform, size, size))
    return 1.0 / float(np.linalg.svd(to_texels, compute_uv=False).max())


def image_source(spec, tint, p, err):
    """-> (src [N, 4] premultiplied and clamped, near [N]): near = a NEAREST sample whose value changes within 4 err of (u, v)."""
    u, v = uv_of(spec, p)
    value = sample(spec, u, v)
    near = np.zeros(len(u), dtype=bool)
    if spec.filter == Filter.Nearest and err > 0.0:
        for du in (-4.0 * err, 4.0 * err):
            for dv in (-4.0 * err, 4.0 * err):
                near |= (sample(spec, u + du, v + dv) != value).any(axis=1)
    t = np.float64(np.float32(tint))
    src = np.concatenate([value[:, :3] * (t[:3] * t[3])[None, :], value[:, 3:4] * t[3]], axis=1)
    return np.clip(np.nan_to_num(src, nan=0.0), 0.0, 1.0), near


def extra_of(spec, err):
    return 2.0 * neighbour_difference(spec) * err if spec.filter == Filter.Linear else 0.0


def model(size, msaa, transforms, colours, regions, paints, s, attachment, background, per_sample=False):
    """paint_model.model with image paints: paints[i] is None (the solid colour), a Paint (a gradient) or an ImageSpec ->
    (expected [H, W, 4] float64 linear, checkable [H, W], the largest extra tolerance term of the paints, the share of the covered pixels
    that only a texel seam makes uncheckable[, the samples' colours [H W, msaa, 4]])."""
    pix = G.samples(size, size, msaa).reshape(-1, 2)
    bg = background.astype(np.float64) / 255.0 if background.dtype == np.uint8 else background
    dst = np.repeat(bg.reshape(-1, 4), msaa, axis=0)
    edge, seams, covered = np.zeros(len(pix), dtype=bool), np.zeros(len(pix), dtype=bool), np.zeros(len(pix), dtype=bool)
    extra = 0.0
    for t, c, region, paint in zip(transforms, colours, regions, paints):
        p = G.to_path(pix, t, size, size)
        sd = region(p) * G.min_pixel_scale(t, size, size)
        edge |= np.abs(sd) <= f32_eps(size, size, 2 * 40.0)
        covered |= sd > 0
        if paint is None:
            tint = np.float64(np.float32(c))
            src = np.tile(np.clip([tint[0] * tint[3], tint[1] * tint[3], tint[2] * tint[3], tint[3]], 0.0, 1.0), (len(pix), 1))
        elif isinstance(paint, ImageSpec):
            u, v = uv_of(paint, p[sd > -1.0])
            err = uv_error(size + 2 * 40.0, texel_px(paint, t, size), float(max(np.abs(u).max(), np.abs(v).max())) if len(u) else 0.0)
            extra = max(extra, extra_of(paint, err))
            src, seam = image_source(paint, c, p, err)
            seams |= seam & (sd > -1.0)
        else:
            dt = M.t_error(size + 2 * 40.0, M.length_px(paint, t, size))
            extra = max(extra, M.max_slope(paint) * dt)
            src, seam = M.paint_source(paint, c, p, 4.0 * dt)
            edge |= seam & (sd > -1.0)  # (a gradient's hard stops are not this module's seams)
        dst = M.blend_src(dst, sd > 0, src, s, attachment)
    expect = dst.reshape(size * size, msaa, 4).mean(axis=1).reshape(size, size, 4)
    by_pixel = lambda a: a.reshape(-1, msaa).any(axis=1)
    seam_only = (by_pixel(seams) & ~by_pixel(edge)).sum() / max(1, by_pixel(covered).sum())
    out = (expect, ~(by_pixel(edge) | by_pixel(seams)).reshape(size, size), extra, float(seam_only))
    return out + (dst.reshape(size * size, msaa, 4),) if per_sample else out


# ---------------------------------------------------------------- images and placements

def random_image(rng, width, height):
    """Premultiplied RGBA8: rgb <= a."""
    a = rng.randint(40, 256, (height, width, 1))
    rgb = np.floor(rng.uniform(0, 1, (height, width, 3)) * (a + 1)).astype(int)
    return np.concatenate([rgb, a], axis=2).astype(np.uint8)


def smooth_image(n=64):
    """A periodic, slowly varying opaque image: neighbouring texels — across the REPEAT seam too — differ by a few codes."""
    j, i = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    c = lambda a: 0.5 + 0.4 * np.cos(2.0 * np.pi * a / n)
    rgb = np.stack([c(i), c(j), c(i + j)], axis=-1)
    return np.concatenate([np.floor(rgb * 255.0 + 0.5), np.full((n, n, 1), 255.0)], axis=2).astype(np.uint8)


def placed(pixels, texel, angle, centre_at, filter, spread_x, spread_y):
    """The image with texels of `texel` path units, turned by `angle`, the path origin at the texel coordinates `centre_at`."""
    c, s = np.cos(angle) / texel, np.sin(angle) / texel
    return ImageSpec(pixels, tuple(float(np.float32(v)) for v in (c, -s, centre_at[0], s, c, centre_at[1])), filter, spread_x, spread_y)


def scene(filter, spread_x, spread_y, seed=5, size=SIZE, n=8):
    """Eight translucent discs and rectangles (tests/test_gpu_blending.py stack) with 5x3 and 8x8 random images in turn: texels of 0.3 path units
    (at least 4.8 pixels: the stack scales a unit to 16 pixels or more), rotated off the axes, the shape's centre near a corner of the image so
    that u and v go negative and beyond the size. Shape 3 has a gradient and shape 5 its solid colour: the table is a mixed one."""
    from test_gpu_blending import stack
    shapes, transforms, colours, regions = stack(seed=seed, size=size, n=n, radius=(16, 36))
    rng = np.random.RandomState(seed + 300)
    images = [random_image(rng, 5, 3), random_image(rng, 8, 8)]
    paints = []
    for i in range(n):
        pixels = images[i % 2]
        h, w = pixels.shape[:2]
        corner = (0.9 * w, 0.1 * h) if i % 4 < 2 else (0.1 * w, 0.9 * h)
        paints.append(placed(pixels, 0.3, rng.uniform(0.3, 1.2), corner, filter, spread_x, spread_y))
    paints[3] = M.random_paint(rng, R.PaintKind.Linear, Spread.Reflect, 3)
    paints[5] = None
    return shapes, transforms, colours, regions, paints


def one_texel_scene(filter):
    from test_gpu_blending import stack
    shapes, transforms, colours, regions = stack(seed=8, size=SIZE, n=4, radius=(16, 36))
    pixel = np.uint8([[[90, 140, 30, 200]]])
    return shapes, transforms, colours, regions, [placed(pixel, 0.3, 0.4 + 0.2 * i, (0.5, 0.5), filter, Spread.Repeat, Spread.Pad) for i in range(4)]


def minified_scene(size=SIZE):
    """A 64x64 smooth image minified to 16 pixels (a texel is a quarter of a pixel), repeated over a rectangle and a disc. One level and no
    mipmaps: the device and the model alias alike, sample by sample."""
    from contrast_renderer_amd import Path
    from test_ground_truth import place
    shapes = [([], [Path.from_rect((0.0, 0.0), (1.0, 0.75))]), ([], [Path.from_circle((0.0, 0.0), 1.0)])]
    regions = [lambda q: G.convex_polygon(q, [(-1, -0.75), (-1, 0.75), (1, 0.75), (1, -0.75)]), lambda q: G.disc(q, (0.0, 0.0), 1.0)]
    transforms = np.float32([place(size, size, 50, 56, 40, rotate=0.3), place(size, size, 84, 80, 32, rotate=-0.5)])
    colours = np.float32([[1.0, 0.9, 0.8, 0.9], [0.8, 1.0, 0.9, 0.7]])
    image = smooth_image(64)
    paints = [placed(image, 16.0 / 64.0 / 40.0, 0.45, (10.0, 20.0), Filter.Linear, Spread.Repeat, Spread.Repeat),
              placed(image, 16.0 / 64.0 / 32.0, -0.8, (40.0, 5.0), Filter.Linear, Spread.Repeat, Spread.Repeat)]
    return shapes, transforms, colours, regions, paints


def grid_cases():
    """(name, scene, sample counts) of every scene test_gpu_image_paints.py holds against model()."""
    out = [(f"{f.name}-{sx.name}-{sy.name}", scene(f, sx, sy), (1, 2, 4, 8)) for f in (Filter.Nearest, Filter.Linear) for sx, sy in SPREADS]
    out += [(f"one-texel-{f.name}", one_texel_scene(f), (4,)) for f in (Filter.Nearest, Filter.Linear)]
    out.append(("minified", minified_scene(), (1, 4)))
    out.append(("blend-states", scene(Filter.Linear, Spread.Reflect, Spread.Repeat, seed=6), (4,)))
    out.append(("srgb", scene(Filter.Linear, Spread.Repeat, Spread.Reflect, seed=9), (4,)))
    return out


# ---------------------------------------------------------------- the cases with an expectation of their own

def recorded_case(size=SIZE):
    """paint_model.recorded_scene with the second cover image painted: a gradient, an image paint and a solid cover inside a clip disc, under an
    opacity group -> (the pieces of recorded_scene with the paints replaced, expected, checkable, extra, seam share)."""
    t_clip, t_all, transforms, colours, group, regions, paints, clip_sd = M.recorded_scene(size)
    image = random_image(np.random.RandomState(12), 8, 8)
    paints = [paints[0], placed(image, 0.3, 0.7, (7.0, 1.0), Filter.Linear, Spread.Reflect, Spread.Repeat), None]
    expect, ok, extra, seams, dst = model(size, 4, transforms, colours, regions, paints, OVER, False, np.zeros((size, size, 4)), per_sample=True)
    # the alpha-context covers are the existing ones: over a cleared frame Scale then Restore leave alpha * a inside the clip
    alpha = dst[:, :, 3]
    expect[..., 3] = np.where((clip_sd > 0).reshape(-1, 4), alpha * group[3], alpha).mean(axis=1).reshape(size, size)
    return (t_clip, t_all, transforms, colours, group, paints), expect, ok, extra, seams


CAMERA_CASES = [(1, Filter.Nearest), (4, Filter.Linear)]


def camera_case(msaa, filter, size=96):
    """The blob of tests/test_perspective_ground_truth.py under its `tilted` camera, image painted (built as the gradient test builds its case) ->
    (transform, colour, spec, expected [size^2, 4], sure [size^2], extra, seam share)."""
    from test_perspective_ground_truth import CASES, blob, camera, ground_truth
    m = np.float32(camera(**CASES["tilted"])).reshape(16)
    image = random_image(np.random.RandomState(31), 5, 3)
    spec = placed(image, 0.5, 0.5, (4.0, 0.5), filter, Spread.Reflect, Spread.Repeat)
    colour = np.float32([1.0, 0.9, 0.8, 0.9])
    offsets = G.SAMPLE_OFFSETS[msaa] - 0.5
    pix = G.pixel_centres(size)
    # the size of a texel on the frame, from the model itself: the largest step of u or v between neighbouring pixels over the blob
    centre = M.to_path_h(pix, m, size)
    u, v = (a.reshape(size, size) for a in uv_of(spec, centre))
    inside = ground_truth(blob(), m, size, [(0.0, 0.0)])[0].reshape(size, size)
    step = max(np.abs(np.diff(a, axis=ax))[(inside[1:] & inside[:-1]) if ax == 0 else (inside[:, 1:] & inside[:, :-1])].max() for a in (u, v) for ax in (0, 1))
    corners = M.to_path_h(np.array([[0.0, 0.0], [size, 0.0], [0.0, size], [size, size]], dtype=np.float64), m, size)
    err = uv_error(float(np.abs(corners).max()) * size + size, 1.0 / step, float(max(np.abs(u[inside]).max(), np.abs(v[inside]).max())))
    delta = 0.02
    expect, sure, seam = np.zeros((size * size, 4)), np.ones(size * size, dtype=bool), np.zeros(size * size, dtype=bool)
    for ox, oy in offsets:
        truth = ground_truth(blob(), m, size, [(ox, oy), (ox + delta, oy + delta), (ox - delta, oy + delta), (ox + delta, oy - delta), (ox - delta, oy - delta)])
        sure &= (truth == truth[0]).all(axis=0)
        src, near = image_source(spec, colour, M.to_path_h(pix + np.array([ox, oy]), m, size), err)
        seam |= near & truth[0]
        expect += np.where(truth[0][:, None], src, 0.0) / len(offsets)
    seams = (seam & sure).sum() / max(1, inside.sum())
    return m, colour, spec, expect, sure & ~seam, extra_of(spec, err), float(seams)


def stroke_case(filter, size=SIZE):
    """The stroke of the gradient tests' case 5, image painted -> (transform, spec, source per pixel centre [size^2, 4], seam [size^2], extra)."""
    from test_ground_truth import place
    t = place(size, size, 64, 64, 56, rotate=0.2)
    spec = placed(random_image(np.random.RandomState(41), 8, 8), 0.1, 0.6, (2.0, 7.0), filter, Spread.Repeat, Spread.Reflect)
    p = G.to_path(G.samples(size, size, 1).reshape(-1, 2), t, size, size)
    u, v = uv_of(spec, p)
    err = uv_error(size + 80.0, texel_px(spec, t, size), float(max(np.abs(u).max(), np.abs(v).max())))
    src, seam = image_source(spec, np.float32([1.0, 1.0, 1.0, 1.0]), p, err)
    return t, spec, src, seam, extra_of(spec, err)


# ---------------------------------------------------------------- the coordinate rule at its ends: exact expectations from the header's text alone

EXTREME_SIZE = 64  # the frame: a power of two, so the blit's inverse homography is exact and (X, Y) = the pixel centres k + 0.5
EXTREME_IMAGE = (8, 5)  # width, height: 2^23 and 2^24 leave other remainders modulo 5 and 10 than modulo 8 and 16
EXTREME_SPREADS = [(Spread.Pad, Spread.Pad), (Spread.Repeat, Spread.Repeat), (Spread.Reflect, Spread.Reflect), (Spread.Repeat, Spread.Reflect)]
LIMIT = 2.0 ** 24
NEUTRAL = 2.0 ** 22


def extreme_rows():
    """(name, own, other, offset): one row of the matrix, coordinate = own * (the row's own axis) + other * (the other axis) + offset. The
    coefficient of the own axis is chosen so that every sum is exact or far from a rounding boundary of f32:
      2^23 - 32 with own = -1: 2^23 - 32 - (k + 0.5) lies below 2^23, where the f32 step is 0.5: exact, and below the clamp;
      2^24 with own = 0: exactly at the clamp; 2^24 + 64 with own = 1: 2^24 + 64 + k + 0.5 rounds to an even integer (the step is 2, a tie
      would be an odd integer) and is clamped; the negatives mirrored; +-3e38 with own = 0 (3e38 + 0.5 is not exact in float64);
      own = 3e38: the product overflows to +inf (1.5e38 in the first column) and is clamped;
      own = 3e38, other = -3e38, offset 1e38: +-inf or +-1e38 and beyond. The product of an fma is not rounded, so inf - inf does not occur for
      a finite matrix and finite (X, Y): NaN reaches the rule through the division of a projective instance only."""
    a, b, c, big = 2.0 ** 23 - 32.0, 2.0 ** 24 - 8.5 + 8.5, 2.0 ** 24 + 64.0, 3e38
    return [("2^23-32", -1.0, 0.0, a), ("-(2^23-32)", 1.0, 0.0, -a), ("2^24", 0.0, 0.0, b), ("-2^24", 0.0, 0.0, -b), ("2^24+64", 1.0, 0.0, c),
            ("-(2^24+64)", -1.0, 0.0, -c), ("3e38", 0.0, 0.0, big), ("-3e38", 0.0, 0.0, -big), ("overflow", big, 0.0, 0.0), ("inf-and-back", big, -big, 1e38)]


def extreme_matrices():
    """(name, (m0 .. m5)): every row of extreme_rows on u, the same on v, and one matrix with another extreme per axis. The other axis of the
    first two is the pixel centre + 2^22: exact where the f32 step is 0.5, so that an f32 error of (X, Y) is rounded away there too — at the
    identity a LINEAR sample sits on the texel centre, where such an error moves floor(v - 0.5) to the texel before with a fraction next to 1."""
    out = [(f"u:{n}", (own, other, c, 0.0, 1.0, NEUTRAL)) for n, own, other, c in extreme_rows()]
    out += [(f"v:{n}", (1.0, 0.0, NEUTRAL, other, own, c)) for n, own, other, c in extreme_rows()]
    rows = {n: (own, other, c) for n, own, other, c in extreme_rows()}
    (uo, ux, uc), (vo, vx, vc) = rows["2^23-32"], rows["-(2^24+64)"]
    return out + [("u:2^23-32,v:-(2^24+64)", (uo, ux, uc, vx, vo, vc))]


def fma32(a, b, c, exact=True):
    """fma(a, b, c) of f32 values held in float64 arrays: the product of two f32 values is exact in float64; the sum is asserted to be (two-sum:
    the error term is zero) unless `exact` is False; one rounding to f32, overflow to inf."""
    a, b, c = (np.asarray(x, dtype=np.float64) for x in (a, b, c))
    assert (np.float64(np.float32(a)) == a).all() and (np.float64(np.float32(b)) == b).all()
    with np.errstate(over="ignore", invalid="ignore"):
        p = a * b
        s = p + c
        if exact:
            finite = np.isfinite(s) & np.isfinite(c)
            t = s - p
            err = np.where(finite, (p - (s - t)) + (c - t), 0.0)
            assert (err == 0.0).all(), "a product-sum that float64 does not hold exactly"
        return np.float64(np.float32(s))


def extreme_uv(matrix, X, Y, exact=True):
    """The header's coordinates: u = fma(Y, m1, fma(X, m0, m2)), v = fma(Y, m4, fma(X, m3, m5)) in f32, NaN -> 0, clamped to +-2^24."""
    m = np.float64(np.float32(matrix))
    u, v = fma32(Y, m[1], fma32(X, m[0], m[2], exact), exact), fma32(Y, m[4], fma32(X, m[3], m[5], exact), exact)
    return tuple(np.clip(np.where(np.isnan(c), 0.0, c), -LIMIT, LIMIT) for c in (u, v))


def extreme_taps(matrix, filter, spread_x, spread_y, size=EXTREME_SIZE, image=EXTREME_IMAGE, scale=(1.0, 1.0), exact=True):
    """-> (i0, i1, j0, j1, fx, fy), each [size, size]: the wrapped indices and the fractions of the filter at every pixel centre scaled by
    `scale` (the perturbation of the stability check). NEAREST: i1 = i0, j1 = j0 and the fractions are 0."""
    w, h = image
    Y, X = np.meshgrid((np.arange(size) + 0.5) * scale[1], (np.arange(size) + 0.5) * scale[0], indexing="ij")
    if scale != (1.0, 1.0):
        X, Y = np.float64(np.float32(X)), np.float64(np.float32(Y))
    u, v = extreme_uv(matrix, X, Y, exact)
    if int(filter) & 1 == int(Filter.Nearest):
        i, j = wrap(np.floor(u).astype(np.int64), w, spread_x), wrap(np.floor(v).astype(np.int64), h, spread_y)
        return i, i, j, j, np.zeros_like(u), np.zeros_like(v)
    a, b = np.float64(np.float32(u - 0.5)), np.float64(np.float32(v - 0.5))
    i, j = np.floor(a).astype(np.int64), np.floor(b).astype(np.int64)
    return wrap(i, w, spread_x), wrap(i + 1, w, spread_x), wrap(j, h, spread_y), wrap(j + 1, h, spread_y), a - i, b - j


def extreme_expectation(pixels, matrix, filter, spread_x, spread_y, size=EXTREME_SIZE):
    """The bytes of the blit under a white tint into a cleared frame. Every case sits on a texel centre (the fractions are 0, asserted), so the
    value is one texel's codes, which decode to k / 255 and encode to k again."""
    h, w = pixels.shape[:2]
    i0, _, j0, _, fx, fy = extreme_taps(matrix, filter, spread_x, spread_y, size, (w, h))
    assert not fx.any() and not fy.any()
    assert i0.min() >= 0 and i0.max() < w and j0.min() >= 0 and j0.max() < h
    return pixels[j0, i0]
