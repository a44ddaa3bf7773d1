"""The generator of the painted fuzz (tests/test_gpu_painted_fuzz.py): test_gpu_fuzz.random_case(seed) as it is — strokes with joins, caps and
dashes, every segment type, perspective through the near plane, depth and cull states, extreme placements, clip nesting, nested opacity groups —
dressed so that it runs through k_raster_paint, k_raster_image, k_raster_mip and k_raster_blend while the oracle is still asked the same solid
question. Each variant rests on a reduction include/contrast_hip.h states:

  gradient, conic   stops that all carry one colour give that colour back exactly, for every t (NaN included);
  image, mip        equal texels give their value back exactly: a white image under the instance colour as tint is the solid colour, for any
                    matrix, filter, spread and level;
  replace           the blend state REPLACE with opaque colours is "over".

Nothing in a variant changes what the oracle is asked: the expectation is oracle.binding.render_pass of variant["case"] — random_case(seed), or
the same with colours[:, 3] = 1 for the replace variants — byte for byte.

Where the colour goes. A painted cover's source is paint(t) * instance colour, so the colour may sit in the stops under a white tint or in the
tint under white stops. The alpha-context covers (Save / Scale / RestoreAlphaContext) do not evaluate a paint: they read the instance colour's
alpha itself — `ca = frag.a0[3]` in csrc/raster_tile_body.inc, `rgba[3]` in render_cover of oracle/raster.hpp — so every instance such a draw names
keeps its colour as the tint and gets white stops. The other instances take one of the two arrangements at random ("tint" / "stops"); with
"stops" the row of the `colors` array handed to the device is (1, 1, 1, 1) and differs from the oracle's: variant["colors"] is the device's
array, variant["case"]["colors"] the oracle's, and the two are never mixed. Image paints always take the colour as tint (texels are white).

No GPU call and no library call in here; every random value comes from a RandomState seeded from `seed`."""
import math

import numpy as np

from contrast_renderer_amd import renderer as R
from contrast_renderer_amd.renderer import PaintKind, Spread
from contrast_renderer_amd.renderer import RenderOperation as Op

import conic_model as CM
import paint_model as M
from test_gpu_fuzz import random_case

VARIANTS = ("gradient", "conic", "image", "mip", "mixed", "replace", "replace+gradient")
SECOND_FORMATS = (R.FORMAT_RGBA8_ATTACHMENT, R.FORMAT_BGRA8, R.FORMAT_BGRA8_ATTACHMENT)
ATTACHMENT_FORMATS = (R.FORMAT_RGBA8_ATTACHMENT, R.FORMAT_BGRA8_ATTACHMENT)  # the expectation takes attachment8=True
BGRA_FORMATS = (R.FORMAT_BGRA8, R.FORMAT_BGRA8_ATTACHMENT)  # the expectation is the RGBA one with channels 0 and 2 swapped
SWAP = [2, 1, 0, 3]
NEAREST, LINEAR, MIPMAP = 0, 1, 0x100
WHITE = (1.0, 1.0, 1.0, 1.0)
SPREADS = (Spread.Pad, Spread.Repeat, Spread.Reflect)
CONTEXT_OPS = (Op.SaveAlphaContext, Op.ScaleAlphaContext, Op.RestoreAlphaContext)
DEFAULT_SEEDS = 48
# test c: the first twelve seeds of the plain (0) and clip (3) kinds that the oracle tessellates (tests/test_painted_fuzz_cpu.py checks the list)
CONSISTENCY_SEEDS = (0, 6, 9, 12, 15, 18, 21, 24, 27, 30, 33, 36)  # (the oracle cannot tessellate seed 3)


def kind_of(seed):
    """random_case's kind: 0 plain, 1 perspective, 2 perspective with depth and cull states, 3 clip nesting, 4 nested opacity groups, 5 extreme placements."""
    return seed % 6


def second_format(seed, variant_index):
    """The format a variant draws into beside FORMAT_RGBA8: every kind (seed % 6) and every variant meets all three over eighteen seeds."""
    return SECOND_FORMATS[(seed // 6 + seed + variant_index) % 3]


def colour_instances(draws):
    """The instances a Color draw names, in order."""
    return sorted({int(d[1]) for d in draws if int(d[2]) == int(Op.Color)})


def context_instances(draws):
    """The instances an alpha-context draw names: their colour's alpha is read as it is."""
    return {int(d[1]) for d in draws if int(d[2]) in [int(op) for op in CONTEXT_OPS]}


def random_stops(rng, colour):
    """1 to 8 stops of one colour at random non-decreasing offsets; about a quarter of the tables have two stops at one offset."""
    n = int(rng.randint(1, 9))
    offsets = np.sort(rng.uniform(0.0, 1.0, n))
    if rng.uniform() < 0.3:
        offsets[0] = 0.0
    if rng.uniform() < 0.3:
        offsets[-1] = 1.0
    if n >= 2 and rng.uniform() < 0.28:
        j = int(rng.randint(1, n))
        offsets[j] = offsets[j - 1]
    return tuple(R.GradientStop(float(np.float32(o)), tuple(float(v) for v in colour)) for o in offsets)


def has_hard_edge(paint):
    return any(a.offset == b.offset for a, b in zip(paint.stops[:-1], paint.stops[1:]))


def random_gradient(rng, kind, colour):
    """paint_model.random_paint or conic_model.random_conic (made for a unit-sized Shape, as scene_mixed's are) scaled by 1/4 .. 4 about the
    origin, so that p0 / p1 lie over and beyond the Shape's extent and some centres inside it, with stops of the one colour."""
    spread = SPREADS[int(rng.randint(0, 3))]
    scale = float(math.exp(rng.uniform(math.log(0.25), math.log(4.0))))
    if kind == PaintKind.Conic:
        fraction = 1.0 if rng.uniform() < 0.25 else float(math.exp(rng.uniform(math.log(0.02), 0.0)))  # a small wedge .. a full turn
        base = CM.random_conic(rng, fraction, spread, n_stops=2, clockwise=bool(rng.randint(0, 2)))
        p0, p1 = tuple(float(np.float32(v * scale)) for v in base.p0), base.p1
    else:
        base = M.random_paint(rng, kind, spread, n_stops=2)
        p0 = tuple(float(np.float32(v * scale)) for v in base.p0)
        p1 = tuple(float(np.float32(v * scale)) for v in base.p1)
    return R.Paint(base.kind, base.spread, p0, p1, random_stops(rng, colour))


def random_image_paint(rng, n_images, filters):
    """layers_model.generate's white_image(): six matrix entries of magnitude 10^-2 .. 10^6, a filter word of `filters`, a spread per axis."""
    return dict(image=int(rng.randint(0, n_images)), matrix=[float(np.float32(v)) for v in rng.uniform(-4, 4, 6) * 10.0 ** rng.randint(-2, 7, 6)],
                filter=int(filters[int(rng.randint(0, len(filters)))]), spreads=[int(v) for v in rng.randint(0, 3, 2)])


def is_image_paint(p):
    return isinstance(p, dict)


def build_variant(rng, name, case, what, solid_share=0.0, may_truncate=False):
    """One table over `case`. what = the kinds a colour-drawn instance may get: "linear", "radial", "conic", "image" (one level, NEAREST or LINEAR),
    "mip" (an image with a chain and CRH_FILTER_MIPMAP), "unflagged" (an image with or without a chain, no flag), "flag-only" (the flag on an image
    without a chain). -> the variant's fields but its name, formats and blending."""
    draws, colours = case["draws"], case["colors"]
    n = len(colours)
    painted, context = colour_instances(draws), context_instances(draws)
    assert painted, "every random_case draws a Color cover"
    images = [dict(size=(int(rng.randint(1, 10)), int(rng.randint(1, 10))), mip=False) for _ in range(int(rng.randint(1, 5)))]  # 1..9 x 1..9 white texels
    with_chain = [k for k in range(len(images)) if k % 2 == 0] if ("mip" in what or "unflagged" in what) else []
    for k in with_chain:
        images[k]["mip"] = True
    table, assoc, arrangement = [], [-1] * n, ["solid"] * n
    device_colours = np.array(colours, dtype=np.float32, copy=True)
    for rank, i in enumerate(painted):
        if rank > 0 and rng.uniform() < solid_share:
            continue
        kind = "mip" if (rank == 0 and "mip" in what) else what[int(rng.randint(0, len(what)))]  # (the first cover of a mip table reads a chain: k_raster_mip runs)
        if kind in ("image", "mip", "unflagged", "flag-only"):
            paint = random_image_paint(rng, len(images), (NEAREST | MIPMAP, LINEAR | MIPMAP) if kind in ("mip", "flag-only") else (NEAREST, LINEAR))
            if kind == "mip":
                paint["image"] = with_chain[int(rng.randint(0, len(with_chain)))]
            elif kind in ("image", "flag-only"):
                flat = [k for k in range(len(images)) if not images[k]["mip"]]
                if not flat:
                    images.append(dict(size=(int(rng.randint(1, 10)), int(rng.randint(1, 10))), mip=False))
                    flat = [len(images) - 1]
                paint["image"] = flat[int(rng.randint(0, len(flat)))]
            arrangement[i] = "tint"
        else:
            in_stops = i not in context and rng.uniform() < 0.5
            arrangement[i] = "stops" if in_stops else "tint"
            paint = random_gradient(rng, {"linear": PaintKind.Linear, "radial": PaintKind.Radial, "conic": PaintKind.Conic}[kind],
                                    tuple(float(v) for v in colours[i]) if in_stops else WHITE)
        assoc[i] = len(table)
        table.append(paint)
    if may_truncate and rng.uniform() < 0.6:  # instances beyond the association are solid: they keep their colour as it is
        first = min(i for i in range(n) if assoc[i] >= 0)
        length = int(rng.randint(first + 1, n + 1))
        for i in range(length, n):
            arrangement[i] = "solid"
        assoc = assoc[:length]
    for i in range(n):
        if arrangement[i] == "stops":
            device_colours[i] = WHITE
    # the reductions' conditions, per instance
    for i in range(n):
        k = assoc[i] if i < len(assoc) else -1
        if arrangement[i] == "solid":
            assert k == -1 and np.array_equal(device_colours[i], colours[i])
        elif arrangement[i] == "tint":
            assert np.array_equal(device_colours[i], colours[i]) and (is_image_paint(table[k]) or all(s.color == WHITE for s in table[k].stops))
        else:
            assert i not in context and tuple(device_colours[i]) == WHITE and all(np.array_equal(np.float32(s.color), colours[i]) for s in table[k].stops)
    assert any(k >= 0 for k in assoc)
    # a painted pass clamps source and result to [0, 1] (include/contrast_hip.h, `source`): the colours lie inside
    assert float(colours.min()) >= 0.0 and float(colours.max()) <= 1.0
    return dict(case=case, table=table, images=images, assoc=assoc, colors=device_colours, arrangement=arrangement)


def variants_of(seed):
    """-> the variants of random_case(seed), in the order of VARIANTS: dict(name, case = what the oracle is asked, blending "over" | "replace",
    formats = (FORMAT_RGBA8, one more), table = [Paint | image paint dict(image, matrix, filter, spreads)], images = [dict(size=(w, h), mip)],
    assoc = the association (instances beyond it are solid), colors = the device's instance colours, arrangement = per instance "solid" | "tint" | "stops")."""
    case = random_case(seed)
    opaque = dict(case, colors=np.array(case["colors"], dtype=np.float32, copy=True))
    opaque["colors"][:, 3] = 1.0
    rng = np.random.RandomState(8100 + seed)
    out = []
    for index, name in enumerate(VARIANTS):
        if name == "gradient":
            v = build_variant(rng, name, case, ("linear", "radial"))
        elif name == "conic":
            v = build_variant(rng, name, case, ("conic",))
        elif name == "image":
            v = build_variant(rng, name, case, ("image",))
        elif name == "mip":
            v = build_variant(rng, name, case, ("mip", "mip", "unflagged", "flag-only", "linear", "radial"))
        elif name == "mixed":
            v = build_variant(rng, name, case, ("linear", "radial", "conic", "image", "mip"), solid_share=1.0 / 3.0, may_truncate=True)
        elif name == "replace":
            v = dict(case=opaque, table=[], images=[], assoc=[], colors=opaque["colors"].copy(), arrangement=["solid"] * len(opaque["colors"]))
        else:
            v = build_variant(rng, name, opaque, ("linear", "radial"))
        v.update(name=name, blending="replace" if name.startswith("replace") else "over", formats=(R.FORMAT_RGBA8, second_format(seed, index)))
        out.append(v)
    return out


def describe(v):
    """A variant as plain comparable values: what the determinism test compares and a failure message may print."""
    return (v["name"], v["blending"], v["formats"], tuple(v["assoc"]), tuple(v["arrangement"]), v["colors"].tobytes(), v["case"]["colors"].tobytes(),
            tuple(repr(p) for p in v["table"]), repr(v["images"]))


def expectation_of(image, fmt):
    """The oracle's RGBA image as a frame of format `fmt` stores it."""
    return image[..., SWAP] if fmt in BGRA_FORMATS else image
