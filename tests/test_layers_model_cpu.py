"""The generator and the host model of the image and layer fuzz (tests/layers_model.py) without a GPU: the conditions that keep the fuzz from
degenerating, its determinism, the blit rule against the float64 model of image paints, and the model's steps against the library's host rules."""
import os
from collections import Counter

import numpy as np
import pytest

from contrast_renderer_amd import renderer as R
from contrast_renderer_amd.renderer import Filter, Spread

import blur_model as BM
import composite_model as CM
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
    by the library's host mirrors: crh_blur_taps, crh_composite_texels, crh_color_filter_texels."""
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
