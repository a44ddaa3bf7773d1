"""tests/painted_fuzz_model.py on the host: the generator is deterministic, the oracle tessellates enough of the default seeds for the GPU test to
mean something, the variants cover what they are meant to cover, and the reductions they rest on hold in the float64 models of the paints."""
from collections import Counter

import numpy as np
import pytest

from contrast_renderer_amd import renderer as R
from contrast_renderer_amd.renderer import PaintKind, Spread

import conic_model as CM
import image_paint_model as IM
import mip_model as MM
import paint_model as M
import painted_fuzz_model as PM
from test_gpu_fuzz import random_case

SEEDS = range(PM.DEFAULT_SEEDS)


@pytest.fixture(scope="module")
def tessellated(oracle_lib):
    """{seed: whether the oracle tessellates random_case(seed)} over the default seeds."""
    from oracle.binding import Oracle
    return {seed: Oracle(random_case(seed)["batch"]).status() == 0 for seed in SEEDS}


@pytest.fixture(scope="module")
def variants(tessellated):
    """[(seed, variant)] of every default seed the GPU test draws."""
    return [(seed, v) for seed in SEEDS if tessellated[seed] for v in PM.variants_of(seed)]


@pytest.mark.parametrize("seed", [4, 21])
def test_the_variants_of_a_seed_are_deterministic(seed):
    first, second = PM.variants_of(seed), PM.variants_of(seed)
    assert [PM.describe(v) for v in first] == [PM.describe(v) for v in second]
    assert [v["name"] for v in first] == list(PM.VARIANTS)
    for v in first:  # and nothing in a variant changes what the oracle is asked
        c, plain = v["case"], random_case(seed)
        assert c["draws"] == plain["draws"] and np.array_equal(c["transforms"], plain["transforms"]) and c["batch"].n_shapes == plain["batch"].n_shapes
        assert np.array_equal(c["colors"][:, :3], plain["colors"][:, :3])
        assert np.array_equal(c["colors"][:, 3], np.ones(len(c["colors"])) if v["blending"] == "replace" else plain["colors"][:, 3])


def test_the_oracle_tessellates_all_but_four_of_the_default_seeds(tessellated):
    """The GPU test skips a seed for one reason only, the one test_random_scene_matches_the_oracle covers: Oracle(batch).status() != 0 (there the
    Scene's status is held against the oracle's). This cap keeps it from passing by skipping."""
    failing = [seed for seed in SEEDS if not tessellated[seed]]
    assert len(SEEDS) - len(failing) >= 42
    assert len(failing) == 4 and sorted(PM.kind_of(s) for s in failing) == [2, 2, 3, 5], failing


def test_the_consistency_seeds_are_the_first_twelve_plain_and_clip_seeds_the_oracle_tessellates(oracle_lib):
    from oracle.binding import Oracle
    found = []
    seed = 0
    while len(found) < 12:
        if PM.kind_of(seed) in (0, 3) and Oracle(random_case(seed)["batch"]).status() == 0:
            found.append(seed)
        seed += 1
    assert tuple(found) == PM.CONSISTENCY_SEEDS


def test_the_default_seeds_cover_what_the_variants_are_for(variants):
    by_kind = Counter((v["name"], PM.kind_of(seed)) for seed, v in variants)
    assert all(by_kind[(name, kind)] >= 1 for name in PM.VARIANTS for kind in range(6)), by_kind
    msaa = Counter((v["name"], v["case"]["msaa"]) for _, v in variants)
    assert all(msaa[(name, m)] >= 1 for name in PM.VARIANTS for m in (1, 4)), msaa
    formats = Counter(v["formats"][1] for _, v in variants)
    assert all(v["formats"][0] == R.FORMAT_RGBA8 for _, v in variants)
    assert all(formats[f] >= 8 for f in PM.SECOND_FORMATS), formats
    gradients = [p for _, v in variants for p in v["table"] if not PM.is_image_paint(p)]
    images = [p for _, v in variants for p in v["table"] if PM.is_image_paint(p)]
    spreads = Counter(int(p.spread) for p in gradients)
    assert all(spreads[int(s)] >= 10 for s in Spread), spreads
    kinds = Counter(int(p.kind) for p in gradients)
    assert all(kinds[int(k)] >= 10 for k in PaintKind), kinds
    stops = Counter(len(p.stops) for p in gradients)
    assert stops[1] >= 5 and stops[8] >= 5, stops
    hard = sum(PM.has_hard_edge(p) for p in gradients)
    assert 0.1 * len(gradients) <= hard <= 0.35 * len(gradients), (hard, len(gradients))
    directions = Counter(CM.table(p)[2] for p in gradients if CM.is_conic(p))
    assert directions[1.0] >= 10 and directions[-1.0] >= 10, directions
    sweeps = [CM.turns_fraction(p) for p in gradients if CM.is_conic(p)]
    assert min(sweeps) < 0.05 and max(sweeps) > 0.999, (min(sweeps), max(sweeps))
    filters = Counter(p["filter"] for p in images)
    assert all(filters[f] >= 10 for f in (PM.NEAREST, PM.LINEAR, PM.NEAREST | PM.MIPMAP, PM.LINEAR | PM.MIPMAP)), filters
    image_spreads = Counter(s for p in images for s in p["spreads"])
    assert all(image_spreads[int(s)] >= 10 for s in Spread), image_spreads
    magnitudes = np.abs(np.float64([m for p in images for m in p["matrix"]]))
    assert magnitudes.min() < 0.04 and magnitudes.max() > 1e6 and all(len(p["matrix"]) == 6 for p in images)
    sizes = {im["size"] for _, v in variants for im in v["images"]}
    assert {w for w, _ in sizes} == set(range(1, 10)) and {h for _, h in sizes} == set(range(1, 10))
    arrangements = Counter(a for _, v in variants for a in v["arrangement"])
    assert arrangements["tint"] >= 100 and arrangements["stops"] >= 100 and arrangements["solid"] >= 100, arrangements


def test_the_tables_of_each_variant_hold_the_paints_it_names(variants):
    shorter = 0
    for seed, v in variants:
        name, table, assoc = v["name"], v["table"], v["assoc"]
        case = v["case"]
        n = len(case["colors"])
        painted = PM.colour_instances(case["draws"])
        used = [table[k] for k in assoc if k >= 0]
        assert len(assoc) <= n and all(-1 <= k < len(table) for k in assoc)
        assert all(assoc[i] == -1 for i in range(len(assoc)) if i not in painted), "a paint acts on the Color operation only"
        flagged = [p for p in used if PM.is_image_paint(p) and p["filter"] & PM.MIPMAP and v["images"][p["image"]]["mip"]]
        if name in ("gradient", "replace+gradient"):
            assert used and all(not PM.is_image_paint(p) and int(p.kind) in (int(PaintKind.Linear), int(PaintKind.Radial)) for p in used)
            assert all(assoc[i] >= 0 for i in painted), "every instance a Color draw names gets a paint"
        elif name == "conic":
            assert used and all(CM.is_conic(p) for p in used) and all(assoc[i] >= 0 for i in painted)
        elif name == "image":
            assert used and all(PM.is_image_paint(p) and p["filter"] in (PM.NEAREST, PM.LINEAR) for p in used) and not any(im["mip"] for im in v["images"])
            assert all(assoc[i] >= 0 for i in painted)
        elif name == "mip":
            assert flagged and assoc[painted[0]] >= 0 and table[assoc[painted[0]]] is flagged[0], "the first painted cover reads a chain"
            assert all(assoc[i] >= 0 for i in painted)
        elif name == "mixed":
            assert used
            shorter += len(assoc) < n
        else:
            assert name == "replace" and table == [] and assoc == []
        # an instance named by an alpha-context draw is never given a white tint (its alpha is what those covers read)
        for i in PM.context_instances(case["draws"]):
            assert v["arrangement"][i] != "stops" and np.array_equal(v["colors"][i], case["colors"][i]), (seed, name, i)
        for i in range(n):
            assert np.array_equal(v["colors"][i], PM.WHITE if v["arrangement"][i] == "stops" else case["colors"][i])
    assert shorter >= 5, shorter
    mixed_kinds = Counter(("image" if PM.is_image_paint(p) else PaintKind(int(p.kind)).name) for _, v in variants if v["name"] == "mixed" for p in v["table"])
    assert all(mixed_kinds[k] >= 5 for k in ("Linear", "Radial", "Conic", "image")), mixed_kinds
    assert sum(-1 in [v["assoc"][i] for i in PM.colour_instances(v["case"]["draws"]) if i < len(v["assoc"])] for _, v in variants if v["name"] == "mixed") >= 10


# ---------------------------------------------------------------- the reductions, in the float64 models

def evaluation_points(rng, centre):
    """Path positions [N, 2]: over the Shape, far outside it, huge, and the paint's own centre (and its neighbours one f32 step away)."""
    c = np.float64(np.float32(centre))
    near = np.float64([np.nextafter(np.float32(c), np.float32(s * 4.0)) for s in (-1.0, 1.0)])
    return np.concatenate([rng.uniform(-2.0, 2.0, (64, 2)), rng.uniform(-1e4, 1e4, (16, 2)), np.float64([[1e30, -1e30], [3e38, 3e38], [-3e38, 1.0], [0.0, 0.0]]),
                           c[None, :], near])


NON_FINITE = np.float64([[np.nan, np.nan], [np.inf, 0.5], [-np.inf, np.inf], [0.25, np.nan], [np.inf, np.inf]])


def premultiplied(colour):
    c = np.float64(np.float32(colour))
    return np.array([c[0] * c[3], c[1] * c[3], c[2] * c[3], c[3]])


def sampled_tables(variants, want, per_variant=3):
    """(seed, variant, instance, paint) of up to per_variant painted instances of every variant, `want` choosing among the paints."""
    for seed, v in variants:
        taken = 0
        for i, k in enumerate(v["assoc"]):
            if k >= 0 and want(v, v["table"][k]) and taken < per_variant:
                taken += 1
                yield seed, v, i, v["table"][k]


def test_gradients_of_one_colour_evaluate_to_the_premultiplied_instance_colour(variants):
    """paint_model.paint_source and conic_model.conic_source of a table's paint, under the colour the device is handed as tint, give the
    premultiplied colour the oracle is asked for — exactly, in float64 — at every position, the paint's centre (turns(0, 0)) and huge
    coordinates included. At a non-finite position too: include/contrast_hip.h (`non-finite`, beside the stops rule) promises that equal stop
    colours give their colour back for every t, NaN included; PAD takes NaN as 0 and REPEAT / REFLECT give the first stop's colour."""
    rng = np.random.RandomState(5)
    checked = Counter()
    for seed, v, i, paint in sampled_tables(variants, lambda v, p: not PM.is_image_paint(p)):
        expect = premultiplied(v["case"]["colors"][i])
        p = np.concatenate([evaluation_points(rng, paint.p0), NON_FINITE])
        with np.errstate(invalid="ignore", over="ignore"):
            if CM.is_conic(paint):
                src, _ = CM.conic_source(paint, v["colors"][i], p, 0.0)
            else:
                src, _ = M.paint_source(paint, v["colors"][i], p, 0.0)
        assert np.array_equal(src, np.tile(expect, (len(p), 1))), (seed, v["name"], i, paint)
        checked[(PaintKind(int(paint.kind)).name, v["arrangement"][i])] += 1
    assert all(checked[(k, a)] >= 5 for k in ("Linear", "Radial", "Conic") for a in ("tint", "stops")), checked


def test_a_nan_t_takes_zero_under_pad_and_the_first_stop_elsewhere():
    """The rule the header states for a gradient parameter that is not a number, with stops that differ: a hard edge at offset 0 shows which."""
    red, green = (1.0, 0.0, 0.0, 1.0), (0.0, 1.0, 0.0, 1.0)
    nan = np.float64([[np.nan, 0.0]])
    for spread, colour in ((Spread.Pad, green), (Spread.Repeat, red), (Spread.Reflect, red)):  # at t = 0 the later stop of a hard edge wins
        paint = R.Paint.linear((0.0, 0.0), (1.0, 0.0), [(0.0, red), (0.0, green), (1.0, green)], spread)
        src, _ = M.paint_source(paint, PM.WHITE, nan, 0.0)
        assert np.array_equal(src[0], np.float64(colour)), spread


def test_white_images_evaluate_to_the_premultiplied_instance_colour(variants):
    """image_paint_model.image_source and mip_model.mip_source of a table's white image under the instance colour as tint: exactly the
    premultiplied colour for any matrix, filter, spread, level and lod. At a non-finite position as well: the image block of
    include/contrast_hip.h says "NaN -> 0, then clamped to +-2^24" for (u, v) and "NaN -> 0" for lod, so every index is a wrapped one."""
    rng = np.random.RandomState(6)
    checked = Counter()
    for seed, v, i, paint in sampled_tables(variants, lambda v, p: PM.is_image_paint(p)):
        expect = premultiplied(v["case"]["colors"][i])
        assert v["arrangement"][i] == "tint"
        w, h = v["images"][paint["image"]]["size"]
        pixels = np.full((h, w, 4), 255, dtype=np.uint8)
        p = np.concatenate([evaluation_points(rng, (0.0, 0.0)), NON_FINITE])
        spec = IM.ImageSpec(pixels, tuple(paint["matrix"]), R.Filter(paint["filter"] & 1), Spread(paint["spreads"][0]), Spread(paint["spreads"][1]))
        with np.errstate(invalid="ignore", over="ignore"):
            if paint["filter"] & PM.MIPMAP and v["images"][paint["image"]]["mip"]:
                levels = MM.chain(pixels)
                assert all((level == 255).all() for level in levels)
                mip = MM.MipSpec(pixels, spec.matrix, paint["filter"], spec.spread_x, spec.spread_y, levels)
                dp = rng.uniform(-1.0, 1.0, (len(p), 2, 2)) * 10.0 ** rng.randint(-6, 7, (len(p), 1, 1))  # any footprint: every lod
                dp[-len(NON_FINITE):] = np.nan
                src, _, _, lod = MM.mip_source(mip, v["colors"][i], p, dp, np.ones(len(p)), 1.0, 1.0, True)
                assert (lod[-len(NON_FINITE):] == 0.0).all()
                checked["mip"] += 1
            else:
                src, _ = IM.image_source(spec, v["colors"][i], p, 0.0)
                checked[int(spec.filter)] += 1
        assert np.array_equal(src, np.tile(expect, (len(p), 1))), (seed, v["name"], i, paint)
    assert checked["mip"] >= 10 and checked[0] >= 10 and checked[1] >= 10, checked
