"""The generator and the host model of the image and layer fuzz (tests/layers_model.py) without a GPU — its kinds: create, snapshot, blur,
composite, color_filter, morphology, convolve, lighting, turbulence, displace, distance_field, resize, mipmaps, the frame and table ops and
the refused calls: the conditions that keep the fuzz from degenerating, its determinism, the blit rule against the float64 model of image paints, and the model's steps against the library's host rules."""
import os
from collections import Counter

import numpy as np
import pytest

from contrast_renderer_amd import renderer as R
from contrast_renderer_amd.renderer import Filter, Spread

import blur_model as BM
import composite_model as CM
import convolve_model as CV
import image_paint_model as IM
import layers_model as L


def _seeds():
    return range(int(os.environ.get("CRH_FUZZ_LAYER_SEEDS", "12")))


@pytest.fixture(scope="module")
def generated(oracle_lib):
    return [L.generate(seed) for seed in range(12)]  # the conditions are stated over the default seeds


def same(a, b):
    if isinstance(a, dict):
        return a.keys() == b.keys() and all(same(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple)):
        return len(a) == len(b) and all(same(x, y) for x, y in zip(a, b))
    if isinstance(a, np.ndarray):
        return isinstance(b, np.ndarray) and a.dtype == b.dtype and np.array_equal(a, b)
    return a == b


def test_the_layer_generator_meets_its_conditions(generated):
    kinds, deep, after_destroy, painted_snapshots, above, below, arrays, dense = Counter(), 0, 0, 0, 0, 0, 0, 0
    residues = {"composite": set(), "color_filter": set()}
    for setup, ops in generated:
        assert 50 <= setup["width"] <= 250 and 40 <= setup["height"] <= 160 and setup["width"] % 16 and setup["height"] % 16 and setup["msaa"] in (1, 4)
        assert sum(1 for op in ops if op["kind"] == "blur" and max(op["sigma"]) == 64.0) <= 1
        for op in ops:
            kind = op["kind"]
            kinds[kind] += 1
            deep += int(kind == "check_image" and op["depth"] >= 3)
            after_destroy += int(kind == "blit" and op["destroyed"])
            painted_snapshots += int(kind == "snapshot" and op["after"] == "painted-cleared")
            if kind == "blur" and op["sigma"][0] > 0.0:
                above, below = above + int(op["width"] > 256), below + int(op["width"] < 256)
            if kind in residues:
                residues[kind].add(op["width"] % 4)
        for _, expect in L.replay_model(setup, ops):
            for a in expect:
                arrays, dense = arrays + 1, dense + int(a.reshape(-1, 4).any(axis=1).mean() > 0.1)
    assert set(kinds) == set(L.KINDS) and min(kinds.values()) >= 3, kinds
    assert deep >= 5 and after_destroy >= 3 and painted_snapshots >= 2, (deep, after_destroy, painted_snapshots)
    assert above >= 2 and below >= 2, (above, below)
    assert residues["composite"] == residues["color_filter"] == {0, 1, 2, 3}, residues
    assert dense >= 0.6 * arrays, (dense, arrays)


def test_the_newer_filters_meet_their_conditions(generated):
    """What keeps morphology, convolve, lighting, turbulence and displace from degenerating inside the sequences: every route and
    instantiation, every edge and operand class, inputs with colours above their alpha, inputs that the device made, sources with a mip
    chain, sources destroyed behind the call, and results that reach a frame — also through a table that outlives them."""
    n = Counter()
    routes, windows, lights = Counter(), Counter(), set()
    five = L.NEW[:5]  # this test's kinds: its counters count them alone (test_distance_and_resize_meet_their_conditions has the two that came later)
    edges = {kind: set() for kind in five if kind != "turbulence"}
    seen = {name: set() for name in ("morphology op", "preserve_alpha", "displace filter", "convolve width", "noise", "stitch", "opaque", "octaves")}
    for setup, ops in generated:
        assert sum(1 for op in ops if op["kind"] == "morphology" and max(op["radius"]) > 64) <= 1
        assert sum(1 for op in ops if op["kind"] == "convolve" and min(op["order"]) > 3 and op["order"][0] * op["order"][1] * op["texels"] > 2000000) <= 1
        for op in ops:
            kind = op["kind"]
            if kind in edges:
                edges[kind].add(op["edge"])
                n[kind, "deep"] += int(op["depth"] >= 2)
                n["mipmapped source"] += int(op["mip"])
            elif kind in L.NEW and kind != "turbulence":
                n[kind, "deep"] += int(op["depth"] >= 2)
            if kind in L.READS and kind != "check_image" and "turbulence" in op["by"]:
                n["turbulence", "deep"] += 1  # its result is consumed
            if kind == "morphology":
                rx, ry = op["radius"]
                assert rx in L.RADII and ry in L.RADII
                routes[L.morphology_route(op["radius"])] += 1
                windows[33 if 2 * ry + 1 <= 33 else 129 if 2 * ry + 1 <= 129 else 385] += int(ry > 0)
                n["wide morphology"] += int(op["width"] > 256 and rx > 0)
                n["straight morphology"] += int(op["straight"][0])
                seen["morphology op"].add(op["op"])
            elif kind == "convolve":
                assert all(1 <= v <= 15 for v in op["order"]) and op["kernel"].shape == (op["order"][1], op["order"][0]) and op["kernel"].dtype == np.float32
                n["order 15"] += int(15 in op["order"])
                n["order 1"] += int(1 in op["order"])
                n["corner target"] += int(op["target"] is not None and op["target"][0] in (0, op["order"][0] - 1) and op["target"][1] in (0, op["order"][1] - 1))
                n["no target"] += int(op["target"] is None)
                n["bias"] += int(op["bias"] != 0.0)
                n["straight convolve"] += int(op["straight"][0])
                seen["preserve_alpha"].add(op["preserve_alpha"])
                seen["convolve width"].add(op["width"] % 4)
            elif kind == "lighting":
                lights.add((op["light"]["kind"], op["op"]))
                n["negative surface_scale"] += int(op["surface_scale"] < 0.0)
            elif kind == "turbulence":
                n["frame-sized noise"] += int(tuple(op["size"]) == (setup["width"], setup["height"]))
                n["negative seed"] += int(op["seed"] < 0)
                n["offset"] += int(op["offset"] != [0.0, 0.0])
                for name in ("noise", "stitch", "opaque", "octaves"):
                    seen[name].add(op[name])
            elif kind == "displace":
                n["self-map"] += int(op["map"] == op["image"])
                n["noise map"] += int(op["by"][1] == "turbulence")
                n["scale 1024"] += int(max(abs(v) for v in op["scale"]) == 1024.0)
                n["scale 0"] += int(op["scale"] == [0.0, 0.0])
                n["straight displace source"] += int(op["straight"][0])
                n["straight displace map"] += int(op["straight"][1])
                seen["displace filter"].add(op["filter"])
            elif kind == "composite":
                n["grown dilate drawn on"] += int(L.GROWN_DILATE in op["via"])
            elif kind in ("blit", "blit_mip", "load_image") and set(op["via"]) & set(five):
                n["reaches a frame"] += 1
                n["reaches a frame destroyed"] += int(kind == "blit" and op["destroyed"])
            elif kind == "destroy_image" and op.get("behind") in five:
                n["source destroyed behind the call"] += 1
    print(dict(n), dict(routes), dict(windows))
    assert set(routes) == set(L.ROUTES) and min(routes.values()) >= 2, routes
    assert set(windows) == {33, 129, 385} and min(windows.values()) >= 1, windows
    assert n["wide morphology"] >= 2 and seen["morphology op"] == {0, 1} and n["grown dilate drawn on"] >= 1, n
    assert all(found == {0, 1, 2, 3} for found in edges.values()), edges
    assert seen["preserve_alpha"] == {False, True} and n["order 15"] >= 1 and n["order 1"] >= 1 and seen["convolve width"] == {0, 1, 2, 3}, (n, seen)
    assert n["corner target"] >= 1 and n["no target"] >= 1 and n["bias"] >= 1, n
    assert len(lights) == 6 and n["negative surface_scale"] >= 1, (lights, n)
    assert n["frame-sized noise"] >= 1 and n["negative seed"] >= 1 and n["offset"] >= 1 and seen["noise"] == {0, 1} and seen["stitch"] == seen["opaque"] == {False, True}, (n, seen)
    assert seen["octaves"] == {0, 1, 2, 3, 4}, seen
    assert n["self-map"] >= 2 and n["noise map"] >= 2 and seen["displace filter"] == {0, 1} and n["scale 1024"] >= 1 and n["scale 0"] >= 1, (n, seen)
    assert min(n["straight morphology"], n["straight convolve"], n["straight displace source"], n["straight displace map"]) >= 1, n
    assert all(n[kind, "deep"] >= 2 for kind in L.NEW), n
    assert n["mipmapped source"] >= 3 and n["reaches a frame"] >= 3 and n["reaches a frame destroyed"] >= 1 and n["source destroyed behind the call"] >= 2, n


def test_distance_and_resize_meet_their_conditions(generated):
    """What keeps distance_field and resize from degenerating inside the sequences, as floors on what the generator feeds them: every mode,
    edge, channel, filter and target class; both sides of launch_image_distance_v's switch of row blocks on results of more than one
    block; the large spreads; grown results composited at their origin; sources wider than k_image_distance_h's segment, straight ones
    read on a colour channel, soft and blobby ones, empty and full ones; straight sources where resize's min(v, alpha) binds, grown
    sources whose origin the result must drop, the half-resolution chain; deep, mipmapped and destroyed sources, results that reach a
    frame, also through a table that outlives them; and the calls the library refuses."""
    n = Counter()
    seen = {name: set() for name in ("mode", "edge", "channel", "filter", "refused")}
    large, targets = Counter(), Counter()
    for setup, ops in generated:
        big = [op["spread"] for op in ops if op["kind"] == "distance_field" and op["spread"] > 64]
        assert len(big) <= 1 and set(big) <= set(L.SPREADS_BIG), big
        large.update(big)
        checked = {op["uid"] for op in ops if op["kind"] == "check_image"}
        for op in ops:
            kind = op["kind"]
            if kind in ("distance_field", "resize"):
                w, h = op["source_size"]
                n[kind, "deep"] += int(op["depth"] >= 2)
                n[kind, "mipmapped source"] += int(op["mip"])
            if kind == "distance_field":
                grown = op["mode"] == 0 and op["edge"] == 0
                assert op["spread"] in L.SPREADS + L.SPREADS_BIG and 1 <= op["threshold"] <= 255
                assert tuple(op["size"]) == ((w + 2 * op["spread"], h + 2 * op["spread"]) if grown else (w, h)) and max(op["size"]) <= 16384
                assert op["spread"] > 64 or max(op["size"]) <= max(L.MAX_SIDE, w, h), op["size"]
                for name in ("mode", "edge", "channel"):
                    seen[name].add(op[name])
                for spread in (16, 17):
                    n["spread", spread, "over 32 rows"] += int(op["spread"] == spread and op["size"][1] > 32)
                n["grown"] += int(grown)
                n["wide source"] += int(w > 256)
                n["straight source on a colour"] += int(op["straight"][0] and op["channel"] != 3)
                n["soft source"] += int(bool({"blur", "turbulence"} & set(op["via"])))
                n["nothing inside"] += int(op["inside"][0] == 0)
                n["everything inside"] += int(op["inside"][0] == op["inside"][1])
            elif kind == "resize":
                assert op["filter"] in range(5) and 1 <= min(op["size"]) and max(op["size"]) <= L.MAX_SIDE, op["size"]
                seen["filter"].add(op["filter"])
                is_class = {"frame": tuple(op["size"]) == (setup["width"], setup["height"]), "small": op["size"][0] <= 40 and op["size"][1] <= 30, "same": tuple(op["size"]) == (w, h),
                            "up and down": (op["size"][0] - w) * (op["size"][1] - h) < 0, "sides": set(op["size"]) <= set(L.RESIZE_SIDES),
                            "half": op.get("chain") in ("down", "up"), "ninth": op.get("chain") == "to a multiple" or (w, h) == (9 * op["size"][0], 9 * op["size"][1])}
                assert is_class[op["target"]], (op["target"], op["size"], op["source_size"])
                targets[op["target"]] += 1
                n["half-resolution chains"] += int(op.get("chain") == "up")
                n["most outputs split a tie, on rough texels"] += int(2 * op["split_ties"] > op["size"][0] + op["size"][1] and op["contrast"] >= 20.0)
                if op["straight"][0]:
                    assert op["min_alpha"] > 0, (setup["seed"], op["size"], op["source_size"])
                    n["straight resize source"] += 1
                n["grown resize source, result checked"] += int(op["source_origin"] != (0, 0) and op["result"] in checked)
            elif kind == "composite":
                n["grown distance drawn on"] += int(L.GROWN_DISTANCE in op["via"] and op["offset"][0] == op["offset"][1] < 0)
            elif kind == "refused":
                assert op["status"] == (L.ERR_UNSUPPORTED if op["sort"] == "taps" else L.ERR_INVALID_ARGUMENT)
                n["refused"] += 1
                seen["refused"].add(op["sort"])
            elif kind == "destroy_image" and op.get("behind") in ("distance_field", "resize"):
                n[op["behind"], "source destroyed behind the call"] += 1
            if kind in ("blit", "blit_mip", "load_image"):
                for made in ("distance_field", "resize"):
                    if made in op["via"]:
                        n[made, "reaches a frame"] += 1
                        n[made, "reaches a frame destroyed"] += int(kind == "blit" and op["destroyed"])
    print(dict(n), dict(large), dict(targets), {name: sorted(found) for name, found in seen.items()})
    assert seen["mode"] == {0, 1} and seen["edge"] == seen["channel"] == {0, 1, 2, 3}, seen
    assert n["spread", 16, "over 32 rows"] >= 1 and n["spread", 17, "over 32 rows"] >= 1, n
    assert set(large) == set(L.SPREADS_BIG), large
    assert n["grown"] >= 3 and n["grown distance drawn on"] >= 2 and n["wide source"] >= 2 and n["straight source on a colour"] >= 2 and n["soft source"] >= 3, n
    assert n["nothing inside"] >= 1 and n["everything inside"] >= 1, n
    assert seen["filter"] == {0, 1, 2, 3, 4} and all(targets[name] >= 2 for name in L.RESIZE_TARGETS), (seen, targets)
    assert n["straight resize source"] >= 2 and n["grown resize source, result checked"] >= 1 and n["half-resolution chains"] >= 2, n
    # the deficit ends between two taps equally near the centre: only the rule's tie order places it, and only a step between the two texels shows it
    assert n["most outputs split a tie, on rough texels"] >= 2, n
    for kind in ("distance_field", "resize"):
        assert n[kind, "deep"] >= 2 and n[kind, "mipmapped source"] >= 1 and n[kind, "source destroyed behind the call"] >= 2, (kind, n)
        assert n[kind, "reaches a frame"] >= 3 and n[kind, "reaches a frame destroyed"] >= 1, (kind, n)
    assert n["refused"] >= 3 and len(seen["refused"]) >= 3, (n, seen)


def host_rule(op, pool):
    """What the library's host function (crh_<filter>_texels) makes of an op of one of the newer kinds on the model's bytes."""
    kind = op["kind"]
    if kind == "turbulence":
        return R.turbulence_texels(op["size"][0], op["size"][1], op["frequency"], op["octaves"], op["seed"], op["noise"], op["stitch"], op["opaque"], op["offset"])
    pixels = pool[op["image"]]["pixels"]
    if kind == "morphology":
        return R.morphology_texels(pixels, op["op"], op["radius"][0], op["radius"][1], op["edge"])
    if kind == "convolve":
        return R.convolve_texels(pixels, op["kernel"], op["divisor"], op["bias"], op["target"], op["edge"], op["preserve_alpha"])
    if kind == "displace":
        return R.displace_texels(pixels, pool[op["map"]]["pixels"], tuple(op["scale"]), op["channels"][0], op["channels"][1], op["filter"], op["edge"])
    if kind == "distance_field":
        return R.distance_texels(pixels, op["spread"], op["mode"], op["channel"], op["threshold"], op["edge"])
    if kind == "resize":
        return R.resize_texels(pixels, op["size"][0], op["size"][1], op["filter"])
    light = op["light"]
    mirror = (R.DistantLight(light["azimuth"], light["elevation"]) if light["kind"] == 0 else R.PointLight(*light["position"]) if light["kind"] == 1 else
              R.SpotLight(tuple(light["position"]), tuple(light["points_at"]), light["spot_exponent"], light["cone_angle"]))
    return R.lighting_texels(pixels, mirror, op["op"], op["surface_scale"], op["constant"], op["specular_exponent"], op["color"], op["edge"])


def test_the_generated_ops_of_the_newer_kinds_equal_the_host_rules(generated, oracle_lib):
    """Every morphology, convolve, lighting, turbulence, displace, distance_field and resize op of the default seeds, with the arguments and
    on the inputs the sequence gives it — grown, filtered, snapshot and straight images among them: the model's bytes are the host rule's, so the library
    accepts every generated call, and a difference on the GPU is the device's."""
    import __graft_entry__ as entry
    entry.build()
    compared = Counter()
    for setup, ops in generated:
        model = L.Model(setup)
        for k, op in enumerate(ops):
            host = host_rule(op, model.pool) if op["kind"] in L.NEW else None
            model.apply(op)
            if host is not None:
                assert np.array_equal(model.pool[-1]["pixels"], host), (setup["seed"], k, {name: value for name, value in op.items() if not isinstance(value, np.ndarray)})
                compared[op["kind"]] += 1
    assert set(compared) == set(L.NEW) and min(compared.values()) >= 3, compared


def test_the_layer_generator_is_deterministic(generated):
    for seed in (0, 5):
        setup, ops = L.generate(seed)
        assert same(setup, generated[seed][0]) and same(ops, generated[seed][1])
        first, second = L.replay_model(setup, ops), L.replay_model(*generated[seed])
        assert same([k for k, _ in first], [k for k, _ in second]) and same([e for _, e in first], [e for _, e in second])


@pytest.mark.parametrize("filter", [Filter.Nearest, Filter.Linear], ids=["nearest", "linear"])
def test_the_blit_rule_is_the_image_paint_model_at_the_identity(filter):
    """At the identity placement pixel (column, row) samples (u, v) = (column + 0.5, row + 0.5): NEAREST floors to the texel, LINEAR has the
    fraction 0 at a texel centre, so the model's value is T[row][column] exactly; under a white tint into a cleared frame the source is the
    result, over content 'over' keeps the old pixel where alpha = 0 and replaces it where alpha = 255."""
    rng = np.random.RandomState(3)
    w, h = 37, 23
    pixels = BM.random_premultiplied(rng, w, h)
    spec = IM.ImageSpec(pixels, (1.0, 0.0, 0.0, 0.0, 1.0, 0.0), filter, Spread.Pad, Spread.Pad)
    j, i = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    p = np.stack([i.reshape(-1) + 0.5, j.reshape(-1) + 0.5], axis=1)
    if filter == Filter.Linear:
        assert not ((p - 0.5) - np.floor(p - 0.5)).any()
    value = IM.sample(spec, *IM.uv_of(spec, p))
    assert np.array_equal(value, pixels.reshape(-1, 4) / 255.0)
    src, _ = IM.image_source(spec, np.float32([1.0, 1.0, 1.0, 1.0]), p, 0.0)
    assert np.array_equal(np.floor(src * 255.0 + 0.5).astype(np.uint8).reshape(h, w, 4), L.blit_bytes(pixels, None))
    binary = L.step_color_filter(pixels, None, L.threshold_tables())
    assert L.binary_alpha(binary) and L.premultiplied(binary) and 0 < (binary[..., 3] == 255).mean() < 1
    old = BM.random_premultiplied(rng, w, h)
    src = binary.reshape(-1, 4) / 255.0
    over = src + old.reshape(-1, 4) / 255.0 * (1.0 - src[:, 3:4])
    assert np.array_equal(np.floor(over * 255.0 + 0.5).astype(np.uint8).reshape(h, w, 4), L.blit_bytes(binary, old))


def test_a_code_decodes_and_encodes_to_itself():
    """What both frame formats do to a loaded byte that a pass leaves alone or replaces: (float)k / 255.0f, times 255 and rounded, is k."""
    k = np.arange(256, dtype=np.float32)
    assert np.array_equal(np.floor(k / np.float32(255.0) * np.float32(255.0) + np.float32(0.5)), k)


def test_the_models_steps_equal_the_librarys_host_rules(oracle_lib):
    """Three chained images — a blur, a composite of it over its source, a colour filter of that — by the Python models the fuzz replays and
    by the library's host mirrors: crh_blur_taps, crh_composite_texels, crh_color_filter_texels; then a chain through the five newer steps, and a distance field and a resize of the same straight texels."""
    import __graft_entry__ as entry
    entry.build()
    rng = np.random.RandomState(8)
    base = L.random_texels(rng, "straight", 21, 13)
    for sigma in L.SIGMAS + (64.0,):
        q, radius = R.blur_taps(sigma)
        assert radius == BM.radius_of(sigma) and [int(v) for v in q] == BM.taps(sigma)[0]
    blurred = L.step_blur(base, 2.5, 0.3, BM.TRANSPARENT)
    assert np.array_equal(blurred, BM.blur(base, R.blur_taps(2.5)[0], R.blur_taps(0.3)[0], BM.TRANSPARENT)) and blurred.shape == (13 + 2, 21 + 16, 4)
    for op in range(13):
        mode, opacity, offset = op % 9, (0.0, 1.0, 0.37)[op % 3], (op - 6, 3 - op)
        composed = L.step_composite(base, blurred, op, mode, opacity, offset)
        placed = CM.place(blurred, 21, 13, *offset)
        host = R.composite_texels(placed.reshape(-1, 4), base.reshape(-1, 4), op, mode, opacity).reshape(13, 21, 4)
        assert np.array_equal(composed, host), (op, mode, opacity)
    tables = rng.randint(0, 256, 1024).astype(np.uint8)
    for matrix, t in ((None, L.threshold_tables()), ([float(np.float32(v)) for v in rng.uniform(-16, 16, 20)], tables), (R.ColorMatrix.saturate(2), None)):
        filtered = L.step_color_filter(composed, matrix, t)
        assert np.array_equal(filtered, R.color_filter_texels(composed.reshape(-1, 4), matrix, t).reshape(composed.shape)), matrix
    # The five newer steps as one chain on the same straight texels — noise of their size, the texels eroded and dilated, convolved,
    # displaced by the noise and by themselves, lit — by the models the fuzz replays and by crh_turbulence_texels, crh_morphology_texels,
    # crh_convolve_texels, crh_displace_texels and crh_lighting_texels.
    assert not L.premultiplied(base)
    for noise_kind, stitch, opaque in ((0, True, False), (1, False, True)):
        how = dict(frequency=[L.f32(0.07), L.f32(0.31)], octaves=3, seed=-5, stitch=stitch, opaque=opaque, offset=[L.f32(3.4), L.f32(-2.25)])
        noise = L.step_turbulence([21, 13], noise=noise_kind, **how)
        assert np.array_equal(noise, R.turbulence_texels(21, 13, how["frequency"], 3, -5, noise_kind, stitch, opaque, how["offset"])), (noise_kind, stitch, opaque)
    for op, radius, edge in ((1, [2, 1], 0), (1, [0, 0], 0), (0, [0, 5], 3), (0, [17, 0], 2), (1, [64, 65], 1)):
        morphed = L.step_morphology(base, op, radius, edge)
        assert np.array_equal(morphed, R.morphology_texels(base, op, radius[0], radius[1], edge)), (op, radius, edge)
        assert morphed.shape == ((13 + 2, 21 + 4, 4) if (op, edge, radius) == (1, 0, [2, 1]) else base.shape)
    morphed = L.step_morphology(base, 0, [1, 1], 1)
    assert not L.premultiplied(morphed)  # colours above their alpha go through: the rule is per channel, with no clamp
    for order, target, bias, edge, preserve_alpha in (((15, 1), None, 0.0, 0, False), ((1, 15), [0, 14], L.f32(0.04), 3, True), ((4, 3), [3, 0], L.f32(-0.07), 2, False)):
        kernel, divisor = CV.random_kernel(rng, *order)
        convolved = L.step_convolve(morphed, kernel, divisor, bias, target, edge, preserve_alpha)
        assert np.array_equal(convolved, R.convolve_texels(morphed, kernel, divisor, bias, target, edge, preserve_alpha)), (order, target)
    for map, scale, channels, filter, edge in ((noise, [1024.0, -1024.0], [0, 1], 0, 2), (noise, [3.25, -7.5], [3, 2], 1, 0), (morphed, [-20.0, 20.0], [0, 3], 1, 3), (base, [0.3, 64.0], [2, 1], 1, 1)):
        displaced = L.step_displace(morphed, map, scale, channels, filter, edge)
        assert np.array_equal(displaced, R.displace_texels(morphed, map, tuple(scale), channels[0], channels[1], filter, edge)), (scale, channels, filter, edge)
    for light, mirror in ((dict(kind=0, azimuth=L.f32(225.5), elevation=L.f32(35.25)), R.DistantLight(L.f32(225.5), L.f32(35.25))),
                          (dict(kind=1, position=[L.f32(6.3), L.f32(7.8), 4.5]), R.PointLight(L.f32(6.3), L.f32(7.8), 4.5)),
                          (dict(kind=2, position=[-2.0, -1.0, 6.0], points_at=[L.f32(12.6), 6.5, 0.0], spot_exponent=3.0, cone_angle=25.0), R.SpotLight((-2.0, -1.0, 6.0), (L.f32(12.6), 6.5, 0.0), 3.0, 25.0))):
        for op, surface_scale in ((0, 3.0), (1, -2.0)):
            how = (surface_scale, L.f32(0.9), 12.0, [1.0, 0.5, L.f32(0.3)], op + 1)
            lit = L.step_lighting(displaced, light, op, *how)
            assert np.array_equal(lit, R.lighting_texels(displaced, mirror, op, *how)), (light, op)
    # The two newest steps on the straight texels: the shape read on a colour channel, as it is (its inside map is not alpha's), and a
    # resize whose min(v, alpha) binds — by the models the fuzz replays and by crh_distance_texels and crh_resize_texels.
    for spread, mode, channel, threshold, edge in ((3, 0, 0, 128, 0), (17, 1, 1, 1, 2), (16, 0, 2, 255, 3), (255, 1, 3, 100, 1)):
        field = L.step_distance_field(base, spread, mode, channel, threshold, edge)
        assert np.array_equal(field, R.distance_texels(base, spread, mode, channel, threshold, edge)), (spread, mode, channel, threshold, edge)
        assert field.shape == ((13 + 2 * spread, 21 + 2 * spread, 4) if (mode, edge) == (0, 0) else base.shape)
    assert not np.array_equal(base[..., 0] >= 128, base[..., 3] >= 128)
    for size, filter in (((21, 13), 4), ((8, 30), 0), ((40, 5), 2), ((1, 1), 3), ((33, 14), 1)):
        counters = {}
        resized = L.step_resize(field if filter == 1 else base, size[0], size[1], filter, counters)
        assert np.array_equal(resized, R.resize_texels(field if filter == 1 else base, size[0], size[1], filter)), (size, filter)
        assert L.premultiplied(resized) and resized.shape == (size[1], size[0], 4) and (filter == 1 or counters["min_alpha"] > 0), (size, filter, counters)
