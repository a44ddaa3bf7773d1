"""The generator and the host model of the stateful image and layer fuzz (tests/test_gpu_layers_fuzz.py): random sequences over one Renderer,
two frames (RGBA8 and RGBA8_ATTACHMENT), a pool of images, a solid Scene and a blit Scene per frame — images created, snapshot from frames,
made of noise, blurred, composited, colour filtered, eroded and dilated, convolved, lit, displaced, turned into distance fields, resized,
mipmapped, loaded back into frames, drawn as image paints through tables that outlive their images, between clears, uploads, plain passes,
re-uploads of the solid Scene and calls that the library refuses. Every image operation has an exact model (blur_model, composite_model,
color_filter_model, morphology_model, convolve_model, lighting_model, turbulence_model, displace_model, distance_model, resize_model,
mip_model) and every pass an exact expectation (the oracle for the solid Scene, the image's own bytes for an identity blit), so every
check is of bytes. No GPU and no library call in here: the oracle alone."""
import numpy as np

from contrast_renderer_amd import scenes

import blur_model as BM
import color_filter_model as FM
import composite_model as CM
import convolve_model as CV
import displace_model as DM
import distance_model as DF
import lighting_model as LM
import mip_model as MM
import morphology_model as MO
import resize_model as RS
import turbulence_model as TM

FORMATS = (0, 2)  # FORMAT_RGBA8, FORMAT_RGBA8_ATTACHMENT: frame 0 and frame 1
MAX_POOL = 8
MAX_SIDE = 300  # a TRANSPARENT blur, dilate or distance field is given another edge when it would grow an image beyond this (the sigma-64 blur, the one radius above 64 and the one spread above 64 apart); no resize has a side above it
SIGMAS = (0.0, 0.01, 0.3, 1.0, 2.5, 6.0)
NEAREST, LINEAR, MIPMAP = 0, 1, 0x100
STENCIL, COLOR = 0, 3  # RenderOperation.Stencil, RenderOperation.Color
KINDS = ("create", "snapshot", "blur", "composite", "color_filter", "mipmaps", "check_image", "destroy_image", "clear", "solid", "upload", "load_image",
         "download", "set_table", "replace_table", "clear_table", "blit", "blit_mip", "white_paint", "reupload",
         "morphology", "convolve", "lighting", "turbulence", "displace", "distance_field", "resize", "refused")
WEIGHTS = (0.06, 0.07, 0.11, 0.09, 0.08, 0.04, 0.08, 0.04, 0.01, 0.09, 0.06, 0.05, 0.06, 0.03, 0.05, 0.04, 0.06, 0.03, 0.03, 0.03,
           0.10, 0.07, 0.07, 0.04, 0.09, 0.10, 0.11, 0.03)
NEW = ("morphology", "convolve", "lighting", "turbulence", "displace", "distance_field", "resize")  # the filters that came after the fuzz was written
READS = ("blur", "composite", "color_filter", "check_image", "load_image", "set_table", "replace_table", "blit_mip") + tuple(k for k in NEW if k != "turbulence")
GROWN_DILATE = "grown dilate"  # beside the kinds in an image's `via`: a DILATE under TRANSPARENT with a non-zero radius is behind it
GROWN_DISTANCE = "grown distance"  # likewise: an OUTSIDE distance field under TRANSPARENT, grown by its spread, is behind it
# the spreads of a distance field: 16 and 17 are the two sides of launch_image_distance_v's switch from 32-row to 128-row blocks (drawn more
# often than the others), and once per seed one of SPREADS_BIG: above 64, above 128 (k_image_distance_h stages more than a segment on either side), the largest
SPREADS = (1, 2, 3, 8, 16, 16, 17, 17, 40, 64)
SPREADS_BIG = (65, 128, 255)
# the sides a resize aims at beside the frame's, the source's and the small ones: round k_image_resize_h's group of 32 output columns,
# its chunk and tile of 64 and k_image_resize_v's block of 32 rows and 64 columns
RESIZE_SIDES = (1, 31, 32, 33, 63, 64, 65, 127, 128, 129)
RESIZE_TARGETS = ("frame", "small", "same", "up and down", "sides")
ERR_UNSUPPORTED, ERR_INVALID_ARGUMENT = 8, 10  # crh_status, what a refused call must raise
REFUSALS = ("spread 0", "spread 256", "threshold 0", "width 0", "height 16385", "filter 5", "taps")  # "taps" needs a pool image with a side above 512
# every route of crh_image_morphology and every instantiation of k_image_morph_v: 0 skips an axis's pass ((0, 0) is the copy), and a vertical
# window 2 radius + 1 of at most 33, at most 129 and above selects one of the three
RADII = (0, 1, 2, 5, 16, 17, 64, 65, 192)
ROUTES = ("copy", "horizontal", "vertical", "both")
DISPLACE_SCALES = ((0.0, 0.0), (1024.0, 1024.0), (-1024.0, -1024.0), (1024.0, -1024.0), (-1024.0, 333.25), (0.0, 37.5), (-20.0, 20.0), (3.25, -7.5), (510.0, 510.0), (0.3, 64.0))


def master_case(seed):
    """The master batch of a seed: scene_mixed, the first of its random seeds the oracle can tessellate (as the lifecycle fuzz picks its own)."""
    from oracle.binding import Oracle
    rng = np.random.RandomState(9300 + seed)
    n = int(rng.randint(10, 20))
    while True:
        sc = scenes.scene_mixed(n, (160, 160), seed=int(rng.randint(0, 100000)))
        if Oracle(sc["batch"]).status() == 0:
            return sc


def threshold_tables():
    """The identity on the colours, alpha to 0 below 128 and to 255 from there: what makes an image one that a blit may draw over content."""
    t = FM.identity_tables().reshape(4, 256).copy()
    t[3] = np.where(np.arange(256) < 128, 0, 255)
    return t.reshape(-1)


def premultiplied(pixels):
    return bool((pixels[..., :3] <= pixels[..., 3:4]).all())


def binary_alpha(pixels):
    return bool(((pixels[..., 3] == 0) | (pixels[..., 3] == 255)).all())


def blit_bytes(pixels, old):
    """The model's blit rule: the identity placement samples texel (column, row) at pixel (column, row) — a NEAREST floor of k + 0.5, a LINEAR
    fraction of 0 — under a white tint: the image's bytes into a cleared frame (old is None); over content, an image of alpha 0 or 255 only:
    its bytes where alpha = 255, the old bytes where alpha = 0. Code k decodes to k / 255 and encodes to k again in both frame formats."""
    if old is None:
        return pixels.copy()
    assert binary_alpha(pixels) and premultiplied(pixels)
    return np.where(pixels[..., 3:4] == 255, pixels, old)


def step_blur(pixels, sigma_x, sigma_y, edge):
    return BM.blur_sigma(pixels, sigma_x, sigma_y, edge)


def step_composite(backdrop, source, op, mode, opacity, offset):
    return CM.composite(backdrop, source, op, mode, CM.opacity_code(opacity), offset[0], offset[1])


def step_color_filter(pixels, matrix, tables):
    return FM.texels(pixels, matrix, tables)


def step_morphology(pixels, op, radius, edge):
    return MO.morphology(pixels, op, radius[0], radius[1], edge)


def step_convolve(pixels, kernel, divisor, bias, target, edge, preserve_alpha):
    return CV.convolve(pixels, kernel, divisor, bias, target, edge, preserve_alpha)


def step_lighting(pixels, light, op, surface_scale, constant, specular_exponent, color, edge):
    """light: the keyword arguments of lighting_model.Light"""
    return LM.lighting(pixels, LM.Light(**light), op, surface_scale, constant, specular_exponent, color, edge)


def step_turbulence(size, frequency, octaves, seed, noise, stitch, opaque, offset):
    return TM.turbulence(size[0], size[1], tuple(frequency), octaves, seed, noise, stitch, opaque, tuple(offset))


def step_displace(pixels, map, scale, channels, filter, edge):
    return DM.displace(pixels, map, tuple(scale), channels[0], channels[1], filter, edge)


def step_distance_field(pixels, spread, mode, channel, threshold, edge):
    return DF.distance_field(pixels, spread, mode, channel, threshold, edge)


def step_resize(pixels, width, height, filter, counters=None):
    return RS.resize(pixels, width, height, filter, counters)


def outline_tables(k, spread):
    """An outline k texels wide of an OUTSIDE distance field: every code from 255 - c(k^2) upward becomes opaque, everything farther
    transparent, on all four channels."""
    return np.tile(np.where(np.arange(256) >= 255 - DF.code(k * k, spread), 255, 0).astype(np.uint8), 4)


def contrast(pixels):
    """The mean step between neighbouring texels along a row, in codes: what a tap moved from one texel to its neighbour can change."""
    return float(np.abs(np.diff(pixels.astype(np.int64), axis=1)).mean()) if pixels.shape[1] > 1 else 0.0


def morphology_route(radius):
    return ROUTES[int(radius[0] > 0) + 2 * int(radius[1] > 0)]


def f32(v):
    return float(np.float32(v))


class Model:
    """What every frame and every pool image must hold. apply(op) -> the arrays the device's answers to the op are compared with (empty for
    an op that checks nothing)."""

    def __init__(self, setup, batch=None, oracle=None):
        from oracle.binding import Oracle
        self.s = setup
        self.batch = master_case(setup["seed"])["batch"] if batch is None else batch
        self.oracle = Oracle(self.batch) if oracle is None else oracle
        w, h = setup["width"], setup["height"]
        self.frame = [dict(image=np.zeros((h, w, 4), np.uint8), cleared=True, last="clear") for _ in FORMATS]
        # dict(pixels, mip, depth, origin, by, via, uid): depth = the device operations behind the image, origin = what Image.origin must be,
        # by = the kind that made it, via = the kinds in its history (and GROWN_DILATE, GROWN_DISTANCE), uid = its number among all images made
        self.pool = []
        self.made = 0
        self.counters = {}  # of the last resize: resize_model's clamp and min(v, alpha) counts
        self.table = [None, None]  # of the blit Scene of each frame: dict(pixels, filter, destroyed, index, via)
        self.slice = tuple(setup["slice"])
        self.instances = None

    def add(self, pixels, by, inputs=(), origin=(0, 0), mark=()):
        """A new pool image made by `by` from the pool entries `inputs`. The origin follows the Image docstrings: blur, dilate and the
        distance field set it, the colour filter, convolve and lighting inherit it (the caller passes the source's), everything else,
        resize too, has (0, 0)."""
        via = frozenset((by,) + tuple(mark)).union(*[e["via"] for e in inputs])
        depth = max([e["depth"] for e in inputs], default=0) + int(by != "create")
        self.pool.append(dict(pixels=pixels, mip=False, depth=depth, origin=tuple(int(v) for v in origin), by=by, via=via, uid=self.made))
        self.made += 1

    def name(self, j, index, filter):
        e = self.pool[index]
        self.table[j] = dict(pixels=e["pixels"], filter=filter, destroyed=False, index=index, via=e["via"])

    # ---- passes
    def solid_pass(self, j, instances):
        from oracle.binding import render_pass
        if instances is not None:
            self.instances = instances
        a, b = self.slice
        t, c = self.instances
        assert len(t) == b - a
        draws = [d for i in range(b - a) for d in ((a + i, i, STENCIL, 0, 0), (a + i, i, COLOR, 0, 0))]
        f = self.frame[j]
        image, _ = render_pass(self.oracle, self.s["width"], self.s["height"], self.s["msaa"], 4, 4, 0, t, c, draws,
                               load=None if f["cleared"] else f["image"], attachment8=FORMATS[j] == 2)
        f.update(image=image, cleared=False, last="solid")

    def blit(self, j):
        f, table = self.frame[j], self.table[j]
        f.update(image=blit_bytes(table["pixels"], None if f["cleared"] else f["image"]), last="painted-cleared" if f["cleared"] else "painted", cleared=False)

    def apply(self, op):
        kind = op["kind"]
        if kind == "create":
            self.add(op["pixels"], kind)
        elif kind == "snapshot":
            self.add(self.frame[op["frame"]]["image"].copy(), kind)
        elif kind == "blur":
            src = self.pool[op["image"]]
            grown = op["edge"] == BM.TRANSPARENT
            self.add(step_blur(src["pixels"], op["sigma"][0], op["sigma"][1], op["edge"]), kind, [src],
                     (BM.radius_of(op["sigma"][0]), BM.radius_of(op["sigma"][1])) if grown else (0, 0))
        elif kind == "composite":
            back, src = self.pool[op["image"]], self.pool[op["source"]]
            self.add(step_composite(back["pixels"], src["pixels"], op["op"], op["mode"], op["opacity"], op["offset"]), kind, [back, src])
        elif kind == "color_filter":
            src = self.pool[op["image"]]
            self.add(step_color_filter(src["pixels"], op["matrix"], op["tables"]), kind, [src], src["origin"])
        elif kind == "morphology":
            src = self.pool[op["image"]]
            grown = MO.grows(op["op"], op["edge"])
            self.add(step_morphology(src["pixels"], op["op"], op["radius"], op["edge"]), kind, [src], op["radius"] if grown else (0, 0),
                     (GROWN_DILATE,) if grown and max(op["radius"]) > 0 else ())
        elif kind == "convolve":
            src = self.pool[op["image"]]
            self.add(step_convolve(src["pixels"], op["kernel"], op["divisor"], op["bias"], op["target"], op["edge"], op["preserve_alpha"]), kind, [src], src["origin"])
        elif kind == "lighting":
            src = self.pool[op["image"]]
            self.add(step_lighting(src["pixels"], op["light"], op["op"], op["surface_scale"], op["constant"], op["specular_exponent"], op["color"], op["edge"]), kind, [src],
                     src["origin"])
        elif kind == "turbulence":
            self.add(step_turbulence(op["size"], op["frequency"], op["octaves"], op["seed"], op["noise"], op["stitch"], op["opaque"], op["offset"]), kind)
        elif kind == "displace":
            src, map = self.pool[op["image"]], self.pool[op["map"]]
            self.add(step_displace(src["pixels"], map["pixels"], op["scale"], op["channels"], op["filter"], op["edge"]), kind, [src, map])
        elif kind == "distance_field":
            src = self.pool[op["image"]]
            grown = DF.grows(op["mode"], op["edge"])
            self.add(step_distance_field(src["pixels"], op["spread"], op["mode"], op["channel"], op["threshold"], op["edge"]), kind, [src],
                     (op["spread"], op["spread"]) if grown else (0, 0), (GROWN_DISTANCE,) if grown else ())
        elif kind == "resize":
            src = self.pool[op["image"]]
            self.counters = {}
            self.add(step_resize(src["pixels"], op["size"][0], op["size"][1], op["filter"], self.counters), kind, [src])
        elif kind == "refused":  # the pool is as it was, and so is the image the call named
            return [self.pool[op["image"]]["pixels"]]
        elif kind == "mipmaps":
            self.pool[op["image"]]["mip"] = True
        elif kind == "check_image":
            e = self.pool[op["image"]]
            assert op["origin"] == e["origin"]
            return MM.chain(e["pixels"]) if e["mip"] else [e["pixels"]]
        elif kind == "destroy_image":
            self.pool.pop(op["image"])
            for table in self.table:
                if table is not None:
                    if table["index"] == op["image"]:
                        table["index"], table["destroyed"] = None, True
                    elif table["index"] is not None and table["index"] > op["image"]:
                        table["index"] -= 1
        elif kind == "clear":
            f = self.frame[op["frame"]]
            f.update(image=np.zeros_like(f["image"]), cleared=True, last="clear")
        elif kind == "solid":
            self.solid_pass(op["frame"], op.get("instances"))
        elif kind == "upload":
            self.frame[op["frame"]].update(image=op["pixels"], cleared=False, last="upload")
        elif kind == "load_image":
            self.frame[op["frame"]].update(image=self.pool[op["image"]]["pixels"].copy(), cleared=False, last="load")
        elif kind == "download":
            return [self.frame[op["frame"]]["image"]]
        elif kind in ("set_table", "replace_table"):
            self.name(op["frame"], op["image"], op["filter"])
        elif kind == "clear_table":
            self.table[op["frame"]] = None
        elif kind == "blit":
            self.blit(op["frame"])
        elif kind == "blit_mip":
            assert self.pool[op["image"]]["mip"]
            self.name(op["frame"], op["image"], op["filter"])
            self.blit(op["frame"])
        elif kind == "white_paint":  # a white image paint is the solid colour, byte for byte; the table is cleared behind the pass
            f = self.frame[op["frame"]]
            last = "painted-cleared" if f["cleared"] else "painted"
            self.solid_pass(op["frame"], op.get("instances"))
            f["last"] = last
        elif kind == "reupload":
            # crh_scene_upload keeps the table and the association of an existing Scene: instance i of the new Shapes has the paint
            # association[i] where the association reaches, none beyond it. The paint is white, so the bytes are the solid pass's; whether the
            # pass is a painted one (the general kernel) follows from the association and the new Shape count: expected_general().
            f = self.frame[op["frame"]]
            general = self.expected_general(op)
            last = ("painted-cleared" if f["cleared"] else "painted") if general else "solid"
            self.slice = tuple(op["slice"])
            self.solid_pass(op["frame"], op["instances"])
            f["last"] = last
        else:
            raise AssertionError(kind)
        return []

    @staticmethod
    def expected_general(op):
        """A re-upload's pass is a painted one when an instance below the new Shape count has a paint: the association is
        [-1] * first + [0] * (length - first)."""
        n = op["slice"][1] - op["slice"][0]
        return int(op["assoc_first"] < min(op["assoc_length"], n))


def random_texels(rng, how, w, h):
    if how == "premultiplied":
        return BM.random_premultiplied(rng, w, h)
    if how == "straight":  # colours above their alpha: loaded with a clamp by compositing and the colour filter, summed as they are by the blur
        t = rng.randint(0, 256, (h, w, 4)).astype(np.uint8)
        t[..., 3] = rng.randint(0, 200, (h, w))
        t[..., 0] = np.maximum(t[..., 0], np.minimum(255, t[..., 3].astype(int) + 1)).astype(np.uint8)
        return t
    if how == "white":
        return np.full((h, w, 4), 255, dtype=np.uint8)
    if how == "checker":
        j, i = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
        return np.repeat(np.where((i + j) % 2 == 0, 255, 0).astype(np.uint8)[:, :, None], 4, axis=2)
    assert how == "alpha0"
    t = rng.randint(0, 256, (h, w, 4)).astype(np.uint8)
    t[..., 3] = 0
    return t


TEXELS = ("premultiplied", "straight", "white", "checker", "alpha0")


def generate(seed):
    """-> (setup, ops): the fixtures of a seed and its op list, which holds every random value the replay needs (texels, matrices, instances).
    The generator runs the model as it goes: what an op may do depends on what the images and frames hold."""
    rng = np.random.RandomState(7300 + seed)
    width, height = int(rng.randint(50, 251)), int(rng.randint(40, 161))
    width -= 1 if width % 16 == 0 else 0
    height -= 1 if height % 16 == 0 else 0
    sc = master_case(seed)
    n_master = sc["batch"].n_shapes

    def new_slice():
        a = int(rng.randint(0, n_master - 2))
        return a, int(rng.randint(a + 2, min(n_master, a + 12) + 1))

    def place(n):
        t = scenes.place(width, height, rng.uniform(0, width, n), rng.uniform(0, height, n), rng.uniform(0.2, 0.7, n) * min(width, height))
        c = np.concatenate([rng.uniform(0, 1, (n, 3)), rng.uniform(0.2, 1, (n, 1))], axis=1).astype(np.float32)
        c[::3, 3] = 1.0
        return t.astype(np.float32), c

    setup = dict(seed=seed, width=width, height=height, msaa=int(rng.choice([1, 4])), slice=new_slice())
    model = Model(setup, sc["batch"])
    ops = []
    big_blur_left = big_morphology_left = heavy_convolve_left = big_distance_left = 1

    def emit(op):
        """Every op that reads pool images also says what they were when it ran: `by` and `straight` per image, in the order image, source,
        map; the union of their `via`; the largest depth; whether the first has mipmaps; the first's uid. A distance_field and a resize also say
        their source's size and origin, their result's size and uid, and what resize_model counted. The conditions of test_layers_model_cpu.py
        read these."""
        if op["kind"] in READS:
            used = [model.pool[op[k]] for k in ("image", "source", "map") if k in op]
            op.update(by=tuple(e["by"] for e in used), straight=tuple(not premultiplied(e["pixels"]) for e in used), via=tuple(sorted(frozenset().union(*[e["via"] for e in used]))),
                      depth=max(e["depth"] for e in used), mip=used[0]["mip"], uid=used[0]["uid"])
            if op["kind"] == "check_image":
                op["origin"] = used[0]["origin"]
            if op["kind"] in ("distance_field", "resize"):
                op.update(source_size=(used[0]["pixels"].shape[1], used[0]["pixels"].shape[0]), source_origin=used[0]["origin"], contrast=contrast(used[0]["pixels"]))
        model.apply(op)
        if op["kind"] in ("distance_field", "resize"):  # which image the result is (a later check_image says which it reads), and what the model counted
            op["result"] = model.pool[-1]["uid"]
            op["size"] = [int(model.pool[-1]["pixels"].shape[1]), int(model.pool[-1]["pixels"].shape[0])]
        if op["kind"] == "resize":
            op.update(min_alpha=model.counters["min_alpha"], split_ties=model.counters["split_ties"])
        ops.append(op)

    def pick(indices):
        return indices[int(rng.randint(0, len(indices)))]

    def a_source(prefer_wide=False):
        """The input of one of the newer filters: mostly any pool image; an image wider than 256, the segment of k_image_morph_h, where asked;
        often one that device operations made, and now and then one that has, or now gets, a mip chain (the filter must read level 0)."""
        pool = model.pool
        wide = [k for k, e in enumerate(pool) if e["pixels"].shape[1] > 256] if prefer_wide else []
        deep = [k for k, e in enumerate(pool) if e["depth"] >= 2]
        straight = [k for k, e in enumerate(pool) if not premultiplied(e["pixels"])]  # colours above their alpha: few images have them, so they are sought
        how = rng.uniform()
        i = pick(straight) if straight and how < 0.15 else pick(wide) if wide and how < 0.8 else pick(deep) if deep and how < 0.9 and rng.uniform() < 0.5 else int(rng.randint(0, len(pool)))
        if not pool[i]["mip"] and rng.uniform() < 0.08:
            emit(dict(kind="mipmaps", image=i))
        return i

    def after_filter(i, kind):
        """Now and then the source is destroyed right behind the call that read it."""
        if rng.uniform() < 0.12:
            emit(dict(kind="destroy_image", image=i, behind=kind))

    def newer(indices):
        """Of the images a frame may show, often one that one of the newer filters is behind."""
        made = [i for i in indices if model.pool[i]["via"].intersection(NEW)]
        return pick(made) if made and rng.uniform() < 0.5 else pick(indices)

    def frame_sized(extra=lambda e: True):
        return [i for i, e in enumerate(model.pool) if e["pixels"].shape[:2] == (height, width) and extra(e)]

    def blittable(j):
        """the pool images a blit into frame j may draw now"""
        over = not model.frame[j]["cleared"]
        return frame_sized(lambda e: premultiplied(e["pixels"]) and (not over or binary_alpha(e["pixels"])))

    def room(n=1):
        while len(model.pool) > MAX_POOL - n:
            emit(dict(kind="destroy_image", image=int(rng.randint(0, len(model.pool)))))

    def white_image():
        return dict(size=(int(rng.randint(1, 10)), int(rng.randint(1, 10))), mip=bool(rng.randint(0, 2)),
                    matrix=[float(np.float32(v)) for v in rng.uniform(-4, 4, 6) * 10.0 ** rng.randint(-2, 7, 6)],
                    filter=int(rng.choice([NEAREST, LINEAR, NEAREST | MIPMAP, LINEAR | MIPMAP])), spreads=[int(v) for v in rng.randint(0, 3, 2)])

    def instances_for(op):
        if model.instances is None or len(model.instances[0]) != model.slice[1] - model.slice[0] or rng.uniform() < 0.4:
            op["instances"] = place(model.slice[1] - model.slice[0])
        return op

    def a_filter():
        return int(rng.choice([NEAREST, LINEAR])) if setup["msaa"] == 1 else NEAREST  # (a LINEAR sample off the pixel centre mixes texels)

    def turbulence_op(size):
        """Noise of a size: mostly a few lattice cells across the image, now and then a frequency of 0 (a constant axis) or up to the limit, 4."""
        frequency = [0.0 if t < 0.1 else f32(rng.uniform(0.3, 4.0)) if t < 0.25 else f32(rng.uniform(0.01, 0.3)) for t in rng.uniform(size=2)]
        return dict(kind="turbulence", size=[int(size[0]), int(size[1])], frequency=frequency, octaves=int(rng.randint(0, 5)), seed=int(rng.randint(-100000, 100000)),
                    noise=int(rng.randint(0, 2)), stitch=bool(rng.randint(0, 2)), opaque=bool(rng.randint(0, 2)),
                    offset=[0.0, 0.0] if rng.uniform() < 0.3 else [f32(v) for v in rng.uniform(-100, 100, 2)])

    n_steps = int(rng.randint(100, 141))
    emit(dict(kind="upload", frame=0, pixels=BM.random_premultiplied(rng, width, height)))  # (the frames show something from the start)
    emit(instances_for(dict(kind="solid", frame=1)))
    while len(ops) < n_steps:
        kind = KINDS[int(rng.choice(len(KINDS), p=np.float64(WEIGHTS) / np.sum(WEIGHTS)))]
        j = int(rng.randint(0, 2))
        pool = model.pool
        if kind == "create" or (not pool and kind in ("blur", "composite", "color_filter", "mipmaps", "check_image", "destroy_image", "morphology", "convolve", "lighting", "displace",
                                                      "distance_field", "resize", "refused")):
            room()
            w, h = (width, height) if rng.uniform() < 0.5 else (int(rng.randint(1, 41)), int(rng.randint(1, 31)))
            how = TEXELS[int(rng.randint(0, len(TEXELS)))]
            emit(dict(kind="create", how=how, pixels=random_texels(rng, how, w, h)))
        elif kind == "snapshot":
            room()
            if model.frame[j]["cleared"] and rng.uniform() < 0.8:
                j = 1 - j  # (mostly of a frame that shows something)
            emit(dict(kind="snapshot", frame=j, after=model.frame[j]["last"]))
        elif kind == "blur":
            room()
            wide = [k for k, e in enumerate(pool) if e["pixels"].shape[1] > 256]  # (k_image_blur_h's row segment is 256 texels)
            i = pick(wide) if wide and rng.uniform() < 0.8 else int(rng.randint(0, len(pool)))
            h, w = pool[i]["pixels"].shape[:2]
            sigma = [float(rng.choice(SIGMAS)), float(rng.choice(SIGMAS))]
            edge = int(rng.randint(0, 4))
            big = bool(big_blur_left and max(w, h) <= 260 and rng.uniform() < 0.4)
            if big:  # once per seed: the largest radius, 192, on one axis
                sigma[int(rng.uniform() < 0.4)] = 64.0
                edge = BM.TRANSPARENT if rng.uniform() < 0.6 else edge
                big_blur_left -= 1
            elif edge == BM.TRANSPARENT and (w + 2 * BM.radius_of(sigma[0]) > MAX_SIDE or h + 2 * BM.radius_of(sigma[1]) > MAX_SIDE):
                edge = int(rng.randint(1, 4))
            if edge == BM.TRANSPARENT and max(w + 2 * BM.radius_of(sigma[0]), h + 2 * BM.radius_of(sigma[1])) > 16384:
                continue  # (the library refuses it)
            emit(dict(kind="blur", image=i, sigma=sigma, edge=edge, width=w))
            if big and pool[-1]["pixels"].shape[1] > 256 and rng.uniform() < 0.7:  # the grown row, wider than k_image_blur_h's segment, blurred along itself
                room()
                emit(dict(kind="blur", image=len(pool) - 1, sigma=[float(rng.choice(SIGMAS[2:])), float(rng.choice(SIGMAS))], edge=int(rng.randint(1, 4)), width=pool[-1]["pixels"].shape[1]))
        elif kind == "composite":
            room()
            sized = frame_sized()
            i = pick(sized) if sized and rng.uniform() < 0.4 else int(rng.randint(0, len(pool)))
            s = i if rng.uniform() < 0.15 else int(rng.randint(0, len(pool)))
            w = pool[i]["pixels"].shape[1]
            emit(dict(kind="composite", image=i, source=s, op=int(rng.randint(0, 13)), mode=int(rng.randint(0, 9)),
                      opacity=float(rng.choice([0.0, 1.0, rng.uniform(), rng.uniform()], p=[0.15, 0.35, 0.25, 0.25])), offset=[int(v) for v in (rng.randint(-w - 3, w + 4, 2) if rng.uniform() < 0.3 else rng.randint(-(w // 4) - 1, w // 4 + 2, 2))], width=w))
        elif kind == "color_filter":
            room()
            sized = frame_sized(lambda e: premultiplied(e["pixels"]))
            how = rng.uniform()
            if how < 0.3 and sized:  # the threshold on alpha: an image a blit may draw over content
                i, matrix, tables = pick(sized), None, threshold_tables()
            else:
                i = int(rng.randint(0, len(pool)))
                listed = FM.matrices()
                matrix = listed[int(rng.randint(0, len(listed)))][1] if how < 0.7 else [float(np.float32(v)) for v in rng.uniform(-FM.MATRIX_MAX, FM.MATRIX_MAX, 20) * rng.choice([1.0, 0.1], 20)]
                tables = rng.randint(0, 256, 1024).astype(np.uint8) if rng.uniform() < 0.4 else None
            emit(dict(kind="color_filter", image=i, matrix=matrix, tables=tables, width=pool[i]["pixels"].shape[1]))
        elif kind == "morphology":
            room(2)
            i = a_source(prefer_wide=True)
            h, w = pool[i]["pixels"].shape[:2]
            mop, edge = int(rng.randint(0, 2)), int(rng.randint(0, 4))
            route = int(rng.choice(4, p=[0.1, 0.25, 0.25, 0.4]))  # ROUTES: bit 0 = a horizontal pass, bit 1 = a vertical one
            radius = [int(rng.choice(RADII[1:7])) if route & 1 else 0, int(rng.choice(RADII[1:7])) if route & 2 else 0]
            big = bool(route and big_morphology_left and max(w, h) <= 260 and rng.uniform() < 0.4)
            if big:  # once per seed: a radius above 64 (65 or the largest, 192) on one axis with a pass
                radius[pick([a for a in (0, 1) if radius[a]])] = int(rng.choice(RADII[7:]))
                big_morphology_left -= 1
            elif MO.grows(mop, edge) and (w + 2 * radius[0] > MAX_SIDE or h + 2 * radius[1] > MAX_SIDE):
                edge = int(rng.randint(1, 4))
            if max(MO.size(w, h, mop, radius[0], radius[1], edge)) > 16384:
                continue  # (the library refuses it)
            emit(dict(kind="morphology", image=i, op=mop, radius=radius, edge=edge, width=w))
            grown = MO.grows(mop, edge) and route
            if big and pool[-1]["pixels"].shape[1] > 256 and rng.uniform() < 0.7:  # the grown row, wider than k_image_morph_h's segment, along itself
                emit(dict(kind="morphology", image=len(pool) - 1, op=int(rng.randint(0, 2)), radius=[int(rng.choice(RADII[1:7])), int(rng.choice(RADII[:4]))], edge=int(rng.randint(1, 4)),
                          width=pool[-1]["pixels"].shape[1]))
            elif grown and rng.uniform() < 0.5:  # an outline's way: the grown result with the image it grew from, placed by its origin
                emit(dict(kind="composite", image=i, source=len(pool) - 1, op=int(rng.randint(0, 13)), mode=int(rng.randint(0, 9)), opacity=float(rng.choice([1.0, rng.uniform()])),
                          offset=[-radius[0], -radius[1]], width=w))
            after_filter(i, kind)
        elif kind == "convolve":
            room()
            i = a_source()
            h, w = pool[i]["pixels"].shape[:2]
            order = [1 if t < 0.15 else 15 if t < 0.3 else int(rng.randint(2, 15)) for t in rng.uniform(size=2)]
            if order[0] * order[1] * w * h > 2000000:  # (the host model's time goes with the taps times the texels: one such call per seed)
                if heavy_convolve_left:
                    heavy_convolve_left -= 1
                else:
                    order[int(order[0] >= order[1])] = int(rng.randint(1, 4))
            kernel, divisor = CV.random_kernel(rng, order[0], order[1])
            t = rng.uniform()
            target = None if t < 0.3 else [int(rng.choice([0, order[0] - 1])), int(rng.choice([0, order[1] - 1]))] if t < 0.6 else [int(rng.randint(0, order[0])), int(rng.randint(0, order[1]))]
            emit(dict(kind="convolve", image=i, kernel=kernel, divisor=divisor, bias=0.0 if rng.uniform() < 0.5 else f32(rng.uniform(-0.1, 0.1)), target=target, edge=int(rng.randint(0, 4)),
                      preserve_alpha=bool(rng.randint(0, 2)), order=order, width=w, texels=w * h))
            after_filter(i, kind)
        elif kind == "lighting":
            room()
            i = a_source()
            h, w = pool[i]["pixels"].shape[:2]
            which = int(rng.randint(0, 3))
            if which == LM.DISTANT:
                light = dict(kind=which, azimuth=f32(rng.uniform(-360, 360)), elevation=f32(rng.uniform(-10, 90)))
            elif which == LM.POINT:  # above the image or a little beside it
                light = dict(kind=which, position=[f32(rng.uniform(-0.2, 1.2) * w), f32(rng.uniform(-0.2, 1.2) * h), f32(rng.uniform(0.5, 0.3 * max(w, h) + 4.0))])
            else:  # from beside a corner into the image, so that the cone's border cuts through it
                light = dict(kind=which, position=[f32(rng.uniform(-0.3, 0.3) * w - 2.0), f32(rng.uniform(-0.3, 0.3) * h - 1.0), f32(rng.uniform(3, 12))],
                             points_at=[f32(rng.uniform(0.2, 0.8) * w), f32(rng.uniform(0.2, 0.8) * h), 0.0],
                             spot_exponent=f32(rng.choice([0.0, 1.0, 3.0, rng.uniform(0, 8)])), cone_angle=f32(rng.choice([0.0, 25.0, 60.0, 90.0, rng.uniform(5, 90)])))
            emit(dict(kind="lighting", image=i, light=light, op=int(rng.randint(0, 2)), surface_scale=f32(rng.uniform(0.5, 8) * rng.choice([1.0, 1.0, -1.0])), constant=f32(rng.uniform(0.3, 2)),
                      specular_exponent=f32(rng.uniform(1, 40)), color=[f32(v) for v in np.minimum(rng.uniform(0, 1.3, 3), 1.0)], edge=int(rng.randint(0, 4)), width=w))
            after_filter(i, kind)
        elif kind == "turbulence":
            room()
            emit(turbulence_op((width, height) if rng.uniform() < 0.5 else (rng.randint(1, 41), rng.randint(1, 31))))
        elif kind == "displace":
            room(2)
            i = a_source()
            h, w = pool[i]["pixels"].shape[:2]
            same = [k for k, e in enumerate(pool) if k != i and e["pixels"].shape == pool[i]["pixels"].shape]
            if rng.uniform() < 0.2:
                m = i  # the source is its own map
            elif same and rng.uniform() < 0.7:
                m = pick(same)
            else:  # the usual map: noise of the source's size
                emit(turbulence_op((w, h)))
                m = len(pool) - 1
            emit(dict(kind="displace", image=i, map=m, scale=list(DISPLACE_SCALES[int(rng.randint(0, len(DISPLACE_SCALES)))]), channels=[int(v) for v in rng.randint(0, 4, 2)],
                      filter=int(rng.randint(0, 2)), edge=int(rng.randint(0, 4)), width=w))
            after_filter(i, kind)
        elif kind == "distance_field":
            outline = rng.uniform() < 0.5  # (what a grown result is followed by, decided here: room() renumbers the pool)
            room(3 if outline else 1)
            soft = [k for k, e in enumerate(pool) if e["via"].intersection(("blur", "turbulence"))]  # soft alpha and blobby shapes: long runs, where the scans of a wave's lanes stop far apart
            straight = [k for k, e in enumerate(pool) if not premultiplied(e["pixels"])]
            sized = frame_sized()  # (a same-size result of one of these is an image the frames take)
            how = rng.uniform()
            i = pick(straight) if straight and how < 0.2 else pick(soft) if soft and 0.2 <= how < 0.4 else pick(sized) if sized and 0.4 <= how < 0.6 else a_source(prefer_wide=True)
            h, w = pool[i]["pixels"].shape[:2]
            spread, mode, edge = int(rng.choice(SPREADS)), int(rng.randint(0, 2)), int(rng.randint(0, 4))
            # the shape's channel: on colours above their alpha mostly a colour, whose inside map is not alpha's
            channel = int(rng.randint(0, 3)) if not premultiplied(pool[i]["pixels"]) and rng.uniform() < 0.7 else int(rng.randint(0, 4))
            threshold = int(rng.choice([1, 128, 255, rng.randint(1, 256)], p=[0.3, 0.3, 0.15, 0.25]))
            if not DF.inside_map(pool[i]["pixels"], channel, threshold).any() and rng.uniform() < 0.7:
                threshold = 1  # (mostly a shape with something in it; none at all where the channel is 0 everywhere)
            big = bool(big_distance_left and max(w, h) <= 260 and rng.uniform() < 0.4)
            if big:  # once per seed: a spread above 64, the three in turn over the seeds (the host model takes up to about 2 s for such a call)
                spread = SPREADS_BIG[seed % len(SPREADS_BIG)]
                big_distance_left -= 1
            elif DF.grows(mode, edge) and max(DF.size(w, h, spread, mode, edge)) > MAX_SIDE:
                edge = int(rng.randint(1, 4))
            if max(DF.size(w, h, spread, mode, edge)) > 16384:
                continue  # (the library refuses it)
            inside = DF.inside_map(pool[i]["pixels"], channel, threshold)
            emit(dict(kind="distance_field", image=i, spread=spread, mode=mode, channel=channel, threshold=threshold, edge=edge, width=w, inside=[int(inside.sum()), int(inside.size)]))
            field = len(pool) - 1
            outline = outline and DF.grows(mode, edge)
            if outline:  # an outline's way: the grown field through a table, then with the image it grew from, placed by its origin
                emit(dict(kind="color_filter", image=len(pool) - 1, matrix=None, tables=outline_tables(int(rng.randint(1, min(spread, 12) + 1)), spread), width=pool[-1]["pixels"].shape[1]))
                emit(dict(kind="composite", image=i, source=len(pool) - 1, op=int(rng.randint(0, 13)), mode=int(rng.randint(0, 9)), opacity=float(rng.choice([1.0, rng.uniform()])),
                          offset=[-spread, -spread], width=w))
            if pool[field]["pixels"].shape[0] * pool[field]["pixels"].shape[1] > 120000:
                # a large spread grew both axes: checked and destroyed at once, since every later reader's host model would pay for its texels
                emit(dict(kind="check_image", image=field, depth=pool[field]["depth"]))
                for k in (field + 1, field) if outline else (field,):
                    emit(dict(kind="destroy_image", image=k))
            after_filter(i, kind)
        elif kind == "resize":
            chain = rng.choice(["half", "ninth", None], p=[0.12, 0.08, 0.8])  # (decided here: room() renumbers the pool)
            room(3 if chain else 1)
            grown = [k for k, e in enumerate(pool) if e["origin"] != (0, 0)]  # the result's origin is (0, 0) whatever the source's is
            i = pick(grown) if grown and rng.uniform() < 0.2 else a_source()
            h, w = pool[i]["pixels"].shape[:2]
            filter = int(rng.randint(0, len(RS.FILTERS)))
            if chain == "half" and 4 <= min(w, h) and max(w, h) <= MAX_SIDE:  # the half-resolution blur: down by about 2, blurred, back up
                half = [(w + 1) // 2, (h + 1) // 2]
                emit(dict(kind="resize", image=i, size=half, filter=filter, target="half", chain="down", width=w))
                emit(dict(kind="blur", image=len(pool) - 1, sigma=[float(rng.choice(SIGMAS[2:5])), float(rng.choice(SIGMAS[2:5]))], edge=int(rng.randint(1, 4)), width=half[0]))
                emit(dict(kind="resize", image=len(pool) - 1, size=[w, h], filter=int(rng.randint(0, len(RS.FILTERS))), target="half", chain="up", width=half[0]))
                after_filter(i, kind)
                continue
            if chain == "ninth":
                # (one unit of one tap moves 1/16384 of the step between two texels: only rough texels show where it went)
                rough = [k for k, e in enumerate(pool) if min(e["pixels"].shape[:2]) >= 45 and contrast(e["pixels"]) >= 40.0]
                if rough:
                    i = pick(rough)
                else:  # none in the pool: random texels, a multiple of 9 on both axes from the start
                    how = TEXELS[int(rng.randint(0, 2))]
                    emit(dict(kind="create", how=how, pixels=random_texels(rng, how, 9 * int(rng.randint(5, 26)), 9 * int(rng.randint(4, 17)))))
                    i = len(pool) - 1
                h, w = pool[i]["pixels"].shape[:2]
                # Down by exactly 9, by way of a multiple of 9 on both axes: every output's centre lies on a texel's centre, the taps on
                # either side of it are pairs at equal distances, and 16384 / 9 leaves BOX a deficit of 4 — the centre, a pair and one tap
                # of the next pair — so every output's taps hang on the rule's "ties to the lower index" (LANCZOS3: most outputs).
                ninth = [int(np.clip((w + 4) // 9, 1, MAX_SIDE // 9)), int(np.clip((h + 4) // 9, 1, MAX_SIDE // 9))]
                if (w, h) != (9 * ninth[0], 9 * ninth[1]):
                    emit(dict(kind="resize", image=i, size=[9 * ninth[0], 9 * ninth[1]], filter=int(rng.choice([RS.BOX, RS.CATMULL_ROM])), target="ninth", chain="to a multiple", width=w))
                    i = len(pool) - 1
                emit(dict(kind="resize", image=i, size=ninth, filter=int(rng.choice([RS.BOX, RS.LANCZOS3])), target="ninth", chain="down by 9", width=9 * ninth[0]))
                after_filter(i, kind)
                continue
            target = RESIZE_TARGETS[int(rng.choice(len(RESIZE_TARGETS), p=[0.28, 0.15, 0.17, 0.2, 0.2]))]
            up = [a for a in (0, 1) if (w, h)[a] < MAX_SIDE and (w, h)[1 - a] > 1]  # the axes that can go up while the other goes down
            if target == "same" and max(w, h) > MAX_SIDE:
                target = "frame"
            if target == "up and down" and not up:
                target = "small"
            up = pick(up) if target == "up and down" else None

            def side(axis, n):
                """a side of the target's class for the axis of n source texels"""
                if target == "frame":  # results that load_image, set_table and the blits take
                    return (width, height)[axis]
                if target == "small":
                    return int(rng.randint(1, (41, 31)[axis]))
                if target == "same":
                    return n
                if target == "sides":
                    return int(rng.choice(RESIZE_SIDES))
                return int(rng.randint(n + 1, min(MAX_SIDE, 2 * n + 2) + 1)) if axis == up else int(rng.randint(1, min(n, MAX_SIDE + 1)))

            size = [side(0, w), side(1, h)]
            for axis, n in enumerate((w, h)):
                while RS.max_count(n, size[axis], filter) > RS.MAX_TAPS:  # (the library refuses it: the axis is drawn again)
                    assert target in ("small", "sides", "up and down")
                    size[axis] = side(axis, n)
            emit(dict(kind="resize", image=i, size=size, filter=filter, target=target, width=w))
            if pool[i]["origin"] != (0, 0):
                emit(dict(kind="check_image", image=len(pool) - 1, depth=pool[-1]["depth"]))
            after_filter(i, kind)
        elif kind == "refused":
            # a call with an argument the header refuses, on a pool image: the status, and nothing else happens
            long = [k for k, e in enumerate(pool) if max(e["pixels"].shape[:2]) > RS.MAX_TAPS]
            sort = REFUSALS[int(rng.randint(0, len(REFUSALS) - (0 if long else 1)))]
            i = pick(long) if sort == "taps" else int(rng.randint(0, len(pool)))
            h, w = pool[i]["pixels"].shape[:2]
            distance, size = dict(spread=4, mode=0, channel=3, threshold=128, edge=1), [8, 8]
            if sort == "taps":  # BOX to one texel along the long side: more than 512 taps
                size = [1, h] if w > RS.MAX_TAPS else [w, 1]
            arguments = {"spread 0": dict(distance, spread=0), "spread 256": dict(distance, spread=256), "threshold 0": dict(distance, threshold=0),
                         "width 0": dict(size=[0, 8], filter=RS.TRIANGLE), "height 16385": dict(size=[8, 16385], filter=RS.TRIANGLE), "filter 5": dict(size=size, filter=5),
                         "taps": dict(size=size, filter=RS.BOX)}[sort]
            emit(dict(kind="refused", image=i, sort=sort, call="distance_field" if "spread" in arguments else "resize", arguments=arguments,
                      status=ERR_UNSUPPORTED if sort == "taps" else ERR_INVALID_ARGUMENT))
        elif kind == "mipmaps":
            emit(dict(kind="mipmaps", image=int(rng.randint(0, len(pool)))))
        elif kind == "check_image":
            deep = [i for i, e in enumerate(pool) if e["depth"] >= 3]
            i = pick(deep) if deep and rng.uniform() < 0.6 else int(rng.randint(0, len(pool)))
            emit(dict(kind="check_image", image=i, depth=pool[i]["depth"]))
        elif kind == "destroy_image":
            named = [t["index"] for t in model.table if t is not None and t["index"] is not None]
            i = pick(named) if named and rng.uniform() < 0.6 else int(rng.randint(0, len(pool)))
            emit(dict(kind="destroy_image", image=i))
        elif kind == "clear":
            emit(dict(kind="clear", frame=j))
        elif kind == "solid":
            emit(instances_for(dict(kind="solid", frame=j)))
        elif kind == "upload":
            emit(dict(kind="upload", frame=j, pixels=BM.random_premultiplied(rng, width, height)))
        elif kind == "load_image":
            sized = frame_sized(lambda e: premultiplied(e["pixels"]))
            if not sized:
                continue
            emit(dict(kind="load_image", frame=j, image=newer(sized)))
        elif kind == "download":
            if model.frame[j]["cleared"] and rng.uniform() < 0.7:
                j = 1 - j
            emit(dict(kind="download", frame=j))
        elif kind in ("set_table", "replace_table"):
            sized = frame_sized(lambda e: premultiplied(e["pixels"]))
            if not sized or (model.table[j] is None) != (kind == "set_table"):
                continue
            binary = [i for i in sized if binary_alpha(pool[i]["pixels"])]
            emit(dict(kind=kind, frame=j, image=pick(binary) if binary and rng.uniform() < 0.5 else newer(sized), filter=a_filter()))
        elif kind == "clear_table":
            if model.table[j] is not None:
                emit(dict(kind="clear_table", frame=j))
        elif kind == "blit":
            if model.table[j] is None:
                sized = frame_sized(lambda e: premultiplied(e["pixels"]))
                if not sized:
                    continue
                emit(dict(kind="set_table", frame=j, image=newer(sized), filter=a_filter()))
            table = model.table[j]
            if table["index"] is not None and rng.uniform() < 0.3:
                emit(dict(kind="destroy_image", image=table["index"]))  # the table keeps the pixels
            if not model.frame[j]["cleared"] and not (binary_alpha(table["pixels"]) and rng.uniform() < 0.8):
                emit(dict(kind="clear", frame=j))
            emit(dict(kind="blit", frame=j, destroyed=table["destroyed"], over=not model.frame[j]["cleared"], via=tuple(sorted(table["via"]))))
        elif kind == "blit_mip":
            if not model.frame[j]["cleared"] and rng.uniform() < 0.5:
                emit(dict(kind="clear", frame=j))
            usable = blittable(j)
            if not usable:
                continue
            i = newer(usable)
            if not pool[i]["mip"]:
                emit(dict(kind="mipmaps", image=i))
            emit(dict(kind="blit_mip", frame=j, image=i, filter=a_filter() | MIPMAP))
        elif kind == "white_paint":
            if rng.uniform() < 0.4 and not model.frame[j]["cleared"]:
                emit(dict(kind="clear", frame=j))
            emit(instances_for(dict(kind="white_paint", frame=j, white=white_image())))
            emit(instances_for(dict(kind="solid", frame=int(rng.randint(0, 2)), after_white=True)))
        else:
            assert kind == "reupload"
            a, b = model.slice if rng.uniform() < 0.4 else new_slice()
            length = int(rng.randint(1, b - a + 5))
            emit(dict(kind="reupload", frame=j, slice=(a, b), assoc_length=length, assoc_first=int(rng.randint(0, length + 1)), white=white_image(), instances=place(b - a)))
    for j in range(2):
        emit(dict(kind="download", frame=j))
    for i in range(len(model.pool)):
        emit(dict(kind="check_image", image=i, depth=model.pool[i]["depth"]))
    return setup, ops


def replay_model(setup, ops):
    """-> [(op index, [expected arrays])] of every op that checks something."""
    model = Model(setup)
    out = []
    for k, op in enumerate(ops):
        expect = model.apply(op)
        if expect:
            out.append((k, expect))
    return out
