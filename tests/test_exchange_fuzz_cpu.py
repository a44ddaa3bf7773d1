"""The generator and the model of the stateful exchange fuzz (tests/exchange_fuzz_model.py) without a GPU: its determinism, the conditions
that keep the fuzz from degenerating, and a replay of every sequence through the model with made-up passes."""
from collections import Counter

import numpy as np
import pytest

import exchange_fuzz_model as F
import exchange_model as M
from exchange_util import same

SEEDS = range(12)


@pytest.fixture(scope="module")
def generated():
    return [F.generate(seed) for seed in SEEDS]


def test_the_exchange_generator_is_deterministic(generated):
    for seed in (0, 7):
        setup, ops = F.generate(seed)
        assert same(setup, generated[seed][0]) and same(ops, generated[seed][1])


def test_the_exchange_generator_meets_its_conditions(generated):
    kinds, as_layer, other_group, size_changes, format_changes, empty, aliased, refused, scans, gathers_after, served_downloads = Counter(), 0, 0, 0, 0, 0, 0, Counter(), Counter(), 0, 0
    for setup, ops in generated:
        (wa, ha), (wb, hb) = setup["sizes"]
        assert 60 <= wa <= 200 and 50 <= ha <= 136 and 20 <= wb <= 120 and 17 <= hb <= 32 and setup["msaa"] in (1, 4)
        pending = set()  # results nobody has looked at
        served = set()
        for op in ops:
            kind = op["kind"]
            kinds[kind] += 1
            if kind == "exchange" and op["fails"]:
                refused[op["why"]] += 1
            elif kind == "exchange":
                as_layer += op["result_as_layer"]
                assert op["result_as_layer"] == len({j for j in op["layers"][1:] if j in pending})
                other_group += int(op["after_other_group"])
                size_changes, format_changes = size_changes + int(op["size_changed"]), format_changes + int(op["format_changed"])
                empty, aliased = empty + int(op["empty_slabs"] > 0), aliased + int(op["aliased"])
                scans[op["scan"]] += 1
                served |= {j for j in op["layers"] if j in pending}
                pending.add(op["result"])
                served.discard(op["result"])
            elif kind == "gather":
                gathers_after += int(op["after_other_group"])
                empty += int(op["empty_slabs"] > 0)
                pending.add(op["result"])
                served.discard(op["result"])
            elif kind == "download":
                # a result is not downloaded before it has served as a layer (the closing downloads of a sequence apart)
                assert op["frame"] not in pending or op["frame"] in served or op.get("final"), op
                served_downloads += int(op["frame"] in pending and op["frame"] in served)
                pending.discard(op["frame"])
            else:
                assert kind in ("upload", "clear", "render", "render_over", "set_rows")
                assert kind != "render_over" or op["frame"] not in pending
                pending.discard(op["frame"])
                served.discard(op["frame"])
    assert set(kinds) == set(F.KINDS) and min(kinds.values()) >= 5, kinds
    assert as_layer >= 10 and other_group >= 3 and size_changes >= 3 and format_changes >= 3 and empty >= 3 and aliased >= 3, (as_layer, other_group, size_changes, format_changes, empty, aliased)
    assert set(refused) == {"sizes", "formats", "a 16F result"} and scans[True] >= 10 and scans[False] >= 10, (refused, scans)
    assert served_downloads >= 5 and gathers_after >= 1, (served_downloads, gathers_after)  # (a gather into a frame the other group's exchange wrote)


def test_every_sequence_replays_through_the_model(generated):
    """With passes made up on the host (random bytes inside the frame's tile rows) every op of every sequence has an expectation of the right
    shape, the refusals are the model's own, and a result is the composite — or the gathered slabs — of what its layers held."""
    for setup, ops in generated:
        rng = np.random.RandomState(setup["seed"])
        model = F.Model(setup)
        rows = {}
        for op in ops:
            observed = None
            if op["kind"] == "set_rows":
                rows[op["frame"]] = op["rows"]
            if op["kind"] in ("render", "render_over"):
                s, fmt = F.FRAMES[op["frame"]]
                w, h = setup["sizes"][s]
                r0, r1 = rows.get(op["frame"], (0, h))
                drawn = M.random_premultiplied(rng, w, h)
                drawn[:r0], drawn[r1:] = 0, 0
                observed = drawn if fmt == F.RGBA8 else (drawn / np.float32(255.0)).astype(np.float16)
                if op["kind"] == "render_over":
                    observed = np.where(M.pixel_nonzero(observed)[..., None], observed, model.bytes[op["frame"]])
            before = [b.copy() for b in model.bytes]
            expect = model.apply(op, observed)
            if op["kind"] == "exchange" and not op["fails"]:
                s = F.FRAMES[op["result"]][0]
                assert {F.FRAMES[j] for j in op["layers"]} in ({(s, F.RGBA8)}, {(s, F.RGBA16F)}) and F.FRAMES[op["result"]][1] == F.RGBA8
                assert np.array_equal(model.bytes[op["result"]], M.composite(np.stack([before[j] for j in op["layers"]])))
                assert len(expect["traffic"]) == F.WORLDS[op["group"]]
                assert rows.get(op["result"], (0, setup["sizes"][s][1])) == (0, setup["sizes"][s][1])  # the exchanges write frames that keep their whole rows
            elif op["kind"] == "exchange":
                assert expect is None and all(np.array_equal(a, b) for a, b in zip(before, model.bytes))
            elif op["kind"] == "gather":
                h = setup["sizes"][F.FRAMES[op["result"]][0]][1]
                for k, (r0, r1) in enumerate(F.slab_rows(h, len(op["layers"]))):
                    assert r0 == r1 or rows.get(op["layers"][k]) == (r0, r1) or (r0, r1) == (0, h)
                    assert np.array_equal(model.bytes[op["result"]][r0:r1], before[op["layers"][k]][r0:r1])
                assert op["result"] not in op["layers"]
            elif op["kind"] == "download":
                assert expect.shape == before[op["frame"]].shape


def test_the_fuzz_slab_rows_are_the_librarys():
    from contrast_renderer_amd import distributed as D
    for height in (1, 17, 32, 50, 136):
        for world in F.WORLDS:
            assert F.slab_rows(height, world) == D.slab_rows(height, world)
