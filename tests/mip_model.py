"""The float64 model of mipmapped image paints (include/contrast_hip.h, crh_image_generate_mipmaps and CRH_FILTER_MIPMAP) and the scenes the mipmap
tests draw: plain numpy over tests/image_paint_model.py, shared by tests/test_mipmaps_cpu.py (the model alone) and tests/test_gpu_mipmaps.py (the
device against it).

The chain is integer arithmetic and is compared bit for bit. The value s(l0) + f (s(l1) - s(l0)) adds two terms to image_paint_model's tolerance:

  per level, 2 D_l uv_error_l — image_paint_model's own term at level l: D_l = the largest channel difference between neighbouring texels of
  level l (wrapped), and uv_error_l = (23 E / tau_l + (3 + 1) U_l) ulp, where a texel of level l is tau_l = tau_0 min(w_0 / w_l, h_0 / h_l)
  pixels wide, the coordinates reach U_l = U max(sx_l, sy_l) and the scale u * sx_l is one more rounding of a value of at most U_l (sx_l itself
  is the f32 the model reads too). The blend weighs the two levels with (1 - f) and f, so the larger of the two terms bounds their sum; the model
  takes the largest over every level a sample reads.

  D_levels lod_error — an error of lod moves f by as much (l0 changes only where f wraps from 1 to 0, and the value is continuous there: both
  sides are s(l0 + 1)), and the value moves by |s(l1) - s(l0)| <= D_levels per unit of f, D_levels = the largest difference the model sees
  between the two levels' samples. lod_error, in units of lod: the entries of J are sums of two products of f32 values — the inverse
  homography's coefficients are stored as f32 (1 ulp each), each product and the sum round once — so an entry is off by at most 3 ulp of the
  sum of its terms' magnitudes; squaring, adding the two squares and the division by W^2 of a projective item are four more relative roundings
  of rho^2, two of rho. With kappa = (the column norm taken over the terms' magnitudes) / rho >= 1, the conditioning of the sums, the relative
  error of rho is at most (3 kappa + 2) ulp for an affine item. A projective item forms h0 - X h6 from the sample's own X, whose error
  image_paint_model bounds by 23 ulp E / s: relative to the entry another 23 (E / s) |h6| / |entry| ulp, which kappa_p = (|h0| + |X h6|) / |h0 - X h6|
  (likewise for the other entries) bounds together with the product's and the difference's rounding when E / s <= |X| + the shape's extent — the
  model takes ROUNDINGS_OF_RHO = 8 for an affine item and 64 for a projective one, times the kappa it measures. log2 turns a relative error e
  of rho into e / ln 2; the hardware logarithm (of rho^2 <= 2^28, halved) is good to one ulp of its result, 14 ulp of lod, and lod - l0 is exact.
  So lod_error = (ROUNDINGS_OF_RHO kappa / ln 2 + 15) ulp.

A NEAREST | MIPMAP sample whose value changes within 4 uv_error_l of its coordinates at either level it reads is a seam and is not checked."""
from collections import namedtuple

import numpy as np

from contrast_renderer_amd import renderer as R
from contrast_renderer_amd.renderer import Filter, Spread

import ground_truth_util as G
import image_paint_model as IM
import paint_model as M
from test_ground_truth import f32_eps

# what an ImagePaint with CRH_FILTER_MIPMAP holds, with the chain on the host: levels[0] is the image, len(levels) == 1 an image without mipmaps
MipSpec = namedtuple("MipSpec", "pixels matrix filter spread_x spread_y levels")
MIPMAP = 0x100
ROUNDINGS_OF_RHO_AFFINE, ROUNDINGS_OF_RHO_PROJECTIVE, ROUNDINGS_OF_LOG = 8, 64, 15
SIZE = IM.SIZE


# ---------------------------------------------------------------- the chain

def level_count(width, height):
    return int(np.floor(np.log2(max(width, height)))) + 1


def downsample(level):
    """[h, w, 4] uint8 -> the level below: (a + b + c + d + 2) >> 2 over the 2 x 2 block, its columns and rows clamped to the level."""
    h, w = level.shape[:2]
    i, j = np.arange(max(1, w >> 1)), np.arange(max(1, h >> 1))
    i0, i1, j0, j1 = np.minimum(2 * i, w - 1), np.minimum(2 * i + 1, w - 1), np.minimum(2 * j, h - 1), np.minimum(2 * j + 1, h - 1)
    t = level.astype(np.int64)
    return ((t[j0][:, i0] + t[j0][:, i1] + t[j1][:, i0] + t[j1][:, i1] + 2) >> 2).astype(np.uint8)


def chain(pixels):
    levels = [np.ascontiguousarray(pixels)]
    while levels[-1].shape[:2] != (1, 1):
        levels.append(downsample(levels[-1]))
    assert len(levels) == level_count(pixels.shape[1], pixels.shape[0])
    return levels


def level_scales(levels):
    """-> [(sx_l, sy_l)]: (float)w_l / (float)w_0 as the host divides, read as float64."""
    h0, w0 = levels[0].shape[:2]
    return [(float(np.float32(l.shape[1]) / np.float32(w0)), float(np.float32(l.shape[0]) / np.float32(h0))) for l in levels]


def mipmapped(spec, filter=None):
    """An ImageSpec -> the MipSpec of the same placement with the whole chain and the filter's MIPMAP flag."""
    return MipSpec(spec.pixels, spec.matrix, int(spec.filter if filter is None else filter) | MIPMAP, spec.spread_x, spec.spread_y, chain(spec.pixels))


def base_spec(spec, level=0):
    return IM.ImageSpec(spec.levels[level], spec.matrix, Filter(int(spec.filter) & 1), spec.spread_x, spec.spread_y)


# ---------------------------------------------------------------- the Jacobian, lod and the two-level blend

def inverse_homography(m, size):
    m = np.float64(m).reshape(16)
    cx, cy, cw = (np.array([m[r], m[4 + r], m[12 + r]]) for r in (0, 1, 3))
    return np.linalg.inv(np.stack([(cx * 0.5 + cw * 0.5) * size, (cw * 0.5 - cy * 0.5) * size, cw]))


def path_jacobian(pix, m, size):
    """-> (p [N, 2], dp [N, 2, 2] with dp[:, a, b] = d p_a / d s_b, kappa [N]): the path position of the frame positions `pix` and its derivative,
    through the float64 inverse homography; kappa = the conditioning of the differences h - X h6 (1 for an affine instance)."""
    h = inverse_homography(m, size)
    q = (h @ np.concatenate([pix, np.ones((len(pix), 1))], axis=1).T).T
    p = q[:, :2] / q[:, 2:3]
    dp, kappa = np.empty((len(pix), 2, 2)), np.ones(len(pix))
    for a in range(2):
        for b in range(2):
            entry = h[a, b] - p[:, a] * h[2, b]
            dp[:, a, b] = entry / q[:, 2]
            with np.errstate(divide="ignore", invalid="ignore"):
                kappa = np.maximum(kappa, np.where(entry != 0.0, (abs(h[a, b]) + np.abs(p[:, a] * h[2, b])) / np.abs(entry), 1.0))
    return p, dp, kappa


def lod_of(spec, dp):
    """-> (lod [N] clamped to [0, L - 1], kappa [N] of the sums du/ds = m0 dp.x/ds + m1 dp.y/ds)."""
    m = np.float64(np.float32(spec.matrix))
    norms, norms_abs = [], []
    for b in range(2):
        du, dv = m[0] * dp[:, 0, b] + m[1] * dp[:, 1, b], m[3] * dp[:, 0, b] + m[4] * dp[:, 1, b]
        au, av = np.abs(m[0] * dp[:, 0, b]) + np.abs(m[1] * dp[:, 1, b]), np.abs(m[3] * dp[:, 0, b]) + np.abs(m[4] * dp[:, 1, b])
        norms.append(np.hypot(du, dv))
        norms_abs.append(np.hypot(au, av))
    rho = np.maximum(norms[0], norms[1])  # (propagates NaN)
    with np.errstate(divide="ignore", invalid="ignore"):
        lod = np.where(rho > 0.0, np.log2(rho), 0.0)
        kappa = np.where(rho > 0.0, np.maximum(norms_abs[0], norms_abs[1]) / rho, 1.0)
    return np.clip(np.nan_to_num(lod, nan=0.0, posinf=np.inf), 0.0, len(spec.levels) - 1.0), kappa


def sample_level(spec, level, u, v):
    sx, sy = level_scales(spec.levels)[level]
    return IM.sample(base_spec(spec, level), u * sx, v * sy)


def sample(spec, u, v, lod):
    """-> ([N, 4] premultiplied value, the levels l0 [N], l1 [N], the samples' largest |s(l1) - s(l0)|)."""
    top = len(spec.levels) - 1
    l0 = np.floor(lod).astype(np.int64)
    f, l1 = (lod - l0)[:, None], np.minimum(l0 + 1, top)
    s0, s1 = np.zeros((len(u), 4)), np.zeros((len(u), 4))
    for level in range(int(l0.min()) if len(l0) else 0, (int(l1.max()) if len(l1) else 0) + 1):
        s = sample_level(spec, level, u, v)
        s0[l0 == level], s1[l1 == level] = s[l0 == level], s[l1 == level]
    return s0 + f * (s1 - s0), l0, l1, float(np.abs(s1 - s0).max()) if len(u) else 0.0


def mip_source(spec, tint, p, dp, kappa_p, extent_px, texel_px, projective, near_only=None):
    """-> (src [N, 4] premultiplied and clamped, near [N], extra, lod [N]): IM.image_source for a MipSpec. near = a NEAREST | MIPMAP sample whose
    value changes within 4 uv_error_l at a level it reads; extra = the tolerance term of the module's docstring over the samples of `near_only`
    (all of them by default)."""
    u, v = IM.uv_of(spec, p)
    lod, kappa = lod_of(spec, dp)
    if len(spec.levels) == 1:
        lod = np.zeros(len(u))
    value, l0, l1, d_levels = sample(spec, u, v, lod)
    seen = np.ones(len(u), dtype=bool) if near_only is None else near_only
    near, extra = np.zeros(len(u), dtype=bool), 0.0
    linear = (int(spec.filter) & 1) == int(Filter.Linear)
    scales = level_scales(spec.levels)
    h0, w0 = spec.levels[0].shape[:2]
    u_max = float(max(np.abs(u[seen]).max(), np.abs(v[seen]).max())) if seen.any() else 0.0
    for level in sorted(set(np.unique(l0[seen])) | set(np.unique(l1[seen]))):
        here = seen & ((l0 == level) | (l1 == level))
        lh, lw = spec.levels[level].shape[:2]
        err = (IM.ROUNDINGS_OF_P * extent_px / (texel_px * min(w0 / lw, h0 / lh)) + (IM.ROUNDINGS_OF_UV + 1) * u_max * max(scales[level])) * G.F32_ULP
        if linear:
            extra = max(extra, 2.0 * IM.neighbour_difference(base_spec(spec, level)) * err)
        else:
            mine = sample_level(spec, level, u[here], v[here])
            moved = np.zeros(int(here.sum()), dtype=bool)
            for du in (-4.0 * err, 4.0 * err):
                for dv in (-4.0 * err, 4.0 * err):
                    moved |= (IM.sample(base_spec(spec, level), u[here] * scales[level][0] + du, v[here] * scales[level][1] + dv) != mine).any(axis=1)
            near[here] |= moved
    if len(spec.levels) > 1 and seen.any():
        roundings = ROUNDINGS_OF_RHO_PROJECTIVE if projective else ROUNDINGS_OF_RHO_AFFINE
        worst = float((kappa * kappa_p)[seen].max())
        extra += d_levels * (roundings * worst / np.log(2.0) + ROUNDINGS_OF_LOG) * G.F32_ULP
    t = np.float64(np.float32(tint))
    src = np.concatenate([value[:, :3] * (t[:3] * t[3])[None, :], value[:, 3:4] * t[3]], axis=1)
    return np.clip(np.nan_to_num(src, nan=0.0), 0.0, 1.0), near, extra, lod


def model(size, msaa, transforms, colours, regions, paints, s, attachment, background):
    """image_paint_model.model with MipSpec paints among the others -> (expected [H, W, 4], checkable [H, W], extra, seam share)."""
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
        if isinstance(paint, MipSpec):
            _, dp, kappa_p = path_jacobian(pix, t, size)
            src, seam, term, _ = mip_source(paint, c, p, dp, kappa_p, size + 2 * 40.0, IM.texel_px(paint, t, size), False, near_only=sd > -1.0)
            extra = max(extra, term)
            seams |= seam & (sd > -1.0)
        elif isinstance(paint, IM.ImageSpec):
            u, v = IM.uv_of(paint, p[sd > -1.0])
            err = IM.uv_error(size + 2 * 40.0, IM.texel_px(paint, t, size), float(max(np.abs(u).max(), np.abs(v).max())) if len(u) else 0.0)
            extra = max(extra, IM.extra_of(paint, err))
            src, seam = IM.image_source(paint, c, p, err)
            seams |= seam & (sd > -1.0)
        elif paint is None:
            tint = np.float64(np.float32(c))
            src = np.tile(np.clip([tint[0] * tint[3], tint[1] * tint[3], tint[2] * tint[3], tint[3]], 0.0, 1.0), (len(pix), 1))
        else:
            dt = M.t_error(size + 2 * 40.0, M.length_px(paint, t, size))
            extra = max(extra, M.max_slope(paint) * dt)
            src, seam = M.paint_source(paint, c, p, 4.0 * dt)
            edge |= seam & (sd > -1.0)
        dst = M.blend_src(dst, sd > 0, src, s, attachment)
    expect = dst.reshape(size * size, msaa, 4).mean(axis=1).reshape(size, size, 4)
    by_pixel = lambda a: a.reshape(-1, msaa).any(axis=1)
    seam_only = (by_pixel(seams) & ~by_pixel(edge)).sum() / max(1, by_pixel(covered).sum())
    return expect, ~(by_pixel(edge) | by_pixel(seams)).reshape(size, size), extra, float(seam_only)


# ---------------------------------------------------------------- images and scenes

def soft_image(rng, width, height):
    """Premultiplied RGBA8 of low contrast — rgb in [64, 192), alpha in [192, 256) — so that a texel of half a pixel stays inside the cap of
    the tolerance's extra term (a neighbour difference of at most 0.5)."""
    return np.concatenate([rng.randint(64, 192, (height, width, 3)), rng.randint(192, 256, (height, width, 1))], axis=2).astype(np.uint8)


def blocky_image(rng, width, height, block):
    """soft_image in blocks of `block` x `block` equal texels: a NEAREST sample's value changes at the blocks' borders only."""
    coarse = soft_image(rng, -(-width // block), -(-height // block))
    return np.ascontiguousarray(np.repeat(np.repeat(coarse, block, axis=0), block, axis=1)[:height, :width])


def checkerboard(n=64):
    """Opaque white and black texels in turn: every level below is uniformly code 128."""
    j, i = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    c = np.where((i + j) % 2 == 0, 255, 0)
    return np.stack([c, c, c, np.full((n, n), 255)], axis=-1).astype(np.uint8)


# minification (texels per pixel along the longer axis of J) of the grid's shapes: between levels, beyond the last level (every sample the
# 1 x 1 texel), and one magnified placement (lod 0: the base filter)
MINIFICATIONS = [1.5, 3.3, 8.0, 200.0, None, 0.4]  # None: the anisotropic placement, 4 x 1.2
ANISOTROPIC = (4.0, 1.2)


def placed_minified(pixels, transform, size, minify, angle, centre_at, filter, spread_x, spread_y, levels=None):
    """An image placed by its size on the frame: J = d(u, v) / d(frame position) = rotation(angle) diag(ku, kv), `minify` = k texels per pixel or
    the pair (ku along the frame's x, kv along its y) of an anisotropic placement — the columns of J have the norms ku and kv. The path origin
    lies at the texel coordinates `centre_at`."""
    ku, kv = (minify, minify) if np.isscalar(minify) else minify
    c, s = np.cos(angle), np.sin(angle)
    a = np.array([[c, -s], [s, c]]) @ np.diag([ku, kv]) @ G.pixel_jacobian(transform, size, size)  # path -> pixels -> texels
    matrix = tuple(float(np.float32(x)) for x in (a[0, 0], a[0, 1], centre_at[0], a[1, 0], a[1, 1], centre_at[1]))
    return MipSpec(pixels, matrix, int(filter), spread_x, spread_y, chain(pixels) if levels is None else levels)


def scene(filter, spread_x, spread_y, seed=5, size=SIZE):
    """Six translucent discs and rectangles (tests/test_gpu_blending.py stack) with a 33 x 17 and a 64 x 64 image in turn at MINIFICATIONS, each
    turned off the axes. LINEAR takes low-contrast random texels and image_paint_model's smooth image; NEAREST the same in blocks, so that its
    seams stay a small share of the covered pixels."""
    from test_gpu_blending import stack
    n = len(MINIFICATIONS)
    shapes, transforms, colours, regions = stack(seed=seed, size=size, n=n, radius=(20, 36))
    rng = np.random.RandomState(seed + 500)
    if (int(filter) & 1) == int(Filter.Linear):
        images = [soft_image(rng, 33, 17), IM.smooth_image(64)]
    else:
        images = [blocky_image(rng, 33, 17, 8), blocky_image(rng, 64, 64, 16)]
    chains = [chain(im) for im in images]
    paints = []
    for i, k in enumerate(MINIFICATIONS):
        pixels = images[i % 2]
        h, w = pixels.shape[:2]
        paints.append(placed_minified(pixels, transforms[i], size, ANISOTROPIC if k is None else k, rng.uniform(0.7, 1.2), (0.4 * w, 0.6 * h), filter, spread_x, spread_y, chains[i % 2]))
    return shapes, transforms, colours, regions, paints


def grid_cases():
    """(name, scene, sample counts) of every scene test_gpu_mipmaps.py holds against model()."""
    out = [(f"LinearMipmap-{sx.name}-{sy.name}", scene(Filter.LinearMipmap, sx, sy), (1, 2, 4, 8)) for sx, sy in IM.SPREADS]
    out += [(f"NearestMipmap-{sx.name}-{sy.name}", scene(Filter.NearestMipmap, sx, sy), (1, 4)) for sx, sy in IM.SPREADS]
    return out


def checkerboard_case(size=SIZE):
    """The 64 x 64 checkerboard under REPEAT, minified 8 x, over one rectangle -> (shapes, transform, colour, region, the MIPMAP spec)."""
    from contrast_renderer_amd import Path
    from test_ground_truth import place
    shapes = [([], [Path.from_rect((0.0, 0.0), (1.0, 0.75))])]
    region = lambda q: G.convex_polygon(q, [(-1, -0.75), (-1, 0.75), (1, 0.75), (1, -0.75)])
    transform = np.float32(place(size, size, 64, 64, 48, rotate=0.3))
    colour = np.float32([0.9, 0.8, 1.0, 1.0])
    spec = placed_minified(checkerboard(64), transform, size, 8.0, 0.45, (10.0, 20.0), Filter.LinearMipmap, Spread.Repeat, Spread.Repeat)
    return shapes, transform, colour, region, spec


def camera_case(msaa, filter=Filter.LinearMipmap, size=96):
    """image_paint_model.camera_case with a mipmapped 64 x 64 smooth image, lod per sample ->
    (transform, colour, spec, expected [size^2, 4], sure [size^2], extra, seam share, the lod range over the shape)."""
    from test_perspective_ground_truth import CASES, blob, camera, ground_truth
    m = np.float32(camera(**CASES["tilted"])).reshape(16)
    image = IM.smooth_image(64)
    plain = IM.placed(image, 1.0 / 24.0, 0.5, (4.0, 0.5), Filter.Linear, Spread.Reflect, Spread.Repeat)
    spec = mipmapped(plain, filter)
    colour = np.float32([1.0, 0.9, 0.8, 0.9])
    offsets = G.SAMPLE_OFFSETS[msaa] - 0.5
    pix = G.pixel_centres(size)
    inside = ground_truth(blob(), m, size, [(0.0, 0.0)])[0]
    p, dp, kappa_p = path_jacobian(pix, m, size)
    u, v = IM.uv_of(spec, p)
    lod_centre, _ = lod_of(spec, dp)
    # the size of a level-0 texel on the frame, at least: 1 / the largest rho over the shape
    rho_max = float(np.exp2(lod_centre[inside].max()))
    corners = M.to_path_h(np.array([[0.0, 0.0], [size, 0.0], [0.0, size], [size, size]], dtype=np.float64), m, size)
    extent = float(np.abs(corners).max()) * size + size
    delta = 0.02
    expect, sure, seam, extra = np.zeros((size * size, 4)), np.ones(size * size, dtype=bool), np.zeros(size * size, dtype=bool), 0.0
    for ox, oy in offsets:
        truth = ground_truth(blob(), m, size, [(ox, oy), (ox + delta, oy + delta), (ox - delta, oy + delta), (ox + delta, oy - delta), (ox - delta, oy - delta)])
        sure &= (truth == truth[0]).all(axis=0)
        p, dp, kappa_p = path_jacobian(pix + np.array([ox, oy]), m, size)
        src, near, term, _ = mip_source(spec, colour, p, dp, kappa_p, extent, 1.0 / rho_max, True, near_only=truth[0])
        extra = max(extra, term)
        seam |= near & truth[0]
        expect += np.where(truth[0][:, None], src, 0.0) / len(offsets)
    seams = (seam & sure).sum() / max(1, inside.sum())
    return m, colour, spec, expect, sure & ~seam, extra, float(seams), float(lod_centre[inside].max() - lod_centre[inside].min())


def stroke_case(size=SIZE):
    """image_paint_model.stroke_case, its image replaced by a 64 x 64 smooth one minified 3 x with LINEAR | MIPMAP ->
    (transform, spec, source per pixel centre [size^2, 4], extra)."""
    from test_ground_truth import place
    t = np.float32(place(size, size, 64, 64, 56, rotate=0.2))
    spec = placed_minified(IM.smooth_image(64), t, size, 3.0, 0.6, (2.0, 7.0), Filter.LinearMipmap, Spread.Repeat, Spread.Reflect)
    pix = G.samples(size, size, 1).reshape(-1, 2)
    p, dp, kappa_p = path_jacobian(pix, t, size)
    src, _, extra, _ = mip_source(spec, np.float32([1.0, 1.0, 1.0, 1.0]), p, dp, kappa_p, size + 80.0, IM.texel_px(spec, t, size), False)
    return t, spec, src, extra
