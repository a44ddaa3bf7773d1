"""Stateful fuzz of the multi-GPU exchange on one device: the op sequences of tests/exchange_fuzz_model.py replayed on one Renderer, ten
frames and two loopback groups (world 3 and 5) that live for the whole sequence. Frames are uploaded, cleared, drawn into (whole, over
content, restricted to tile rows), exchanged as layers of either group at any rank and written as results — also a frame that is a layer of
the same call — and gathered slab by slab. A result is what the host model composites from what its layers held, byte for byte, and it is
looked at only after it has been a layer of a later exchange: nothing in between waits for the exchange that wrote it, so the streams of
the communicators have to be ordered behind each other's writes on the device."""
import os

import numpy as np
import pytest

from contrast_renderer_amd import renderer as R

import exchange_fuzz_model as F
import exchange_model as M
from exchange_util import assert_traffic, rect_scene

pytestmark = pytest.mark.gpu


def _seeds():
    return range(int(os.environ.get("CRH_FUZZ_EXCHANGE_SEEDS", "12")))


def describe(op):
    return {k: (f"<{v.dtype} {v.shape}>" if isinstance(v, np.ndarray) else v) for k, v in op.items()}


@pytest.mark.parametrize("seed", _seeds())
def test_random_exchange_sequences_against_a_host_model(seed, monkeypatch):
    import torch
    assert torch.cuda.is_available()
    setup, ops = F.generate(seed)
    model = F.Model(setup)
    r = R.Renderer(R.Configuration(setup["msaa"], 4, 4), device=0)
    frames = [R.Frame(r, *setup["sizes"][s], R.FORMAT_RGBA16F if fmt == F.RGBA16F else R.FORMAT_RGBA8) for s, fmt in F.FRAMES]
    scenes = [[rect_scene(r, *size, spec["rects"]) + (spec["colors"],) for spec in setup["scenes"][s]] for s, size in enumerate(setup["sizes"])]
    groups = []
    for world in F.WORLDS:
        comms = [R.Comm(r, 0, world)]
        comms += [R.Comm(r, k, world, rank0=comms[0]) for k in range(1, world)]
        groups.append(comms)
    rows = {}
    for step, op in enumerate(ops):
        kind = op["kind"]
        where = f"seed {seed} op {step} {describe(op)}"
        if kind == "upload":
            frames[op["frame"]].upload(op["pixels"])
            model.apply(op)
        elif kind == "clear":
            frames[op["frame"]].clear()
            model.apply(op)
        elif kind == "set_rows":
            frames[op["frame"]].set_tile_rows(*op["rows"])
            rows[op["frame"]] = op["rows"]
            model.apply(op)
        elif kind in ("render", "render_over"):
            frame = frames[op["frame"]]
            scene, t, colors = scenes[F.FRAMES[op["frame"]][0]][op["scene"]]
            scene.render(frame, t, colors)
            drawn = frame.download()  # the pass's own answer is the model's: the exchange is what is checked
            r0, r1 = rows.get(op["frame"], (0, frame.height))
            if kind == "render":
                assert not drawn[:r0].any() and not drawn[r1:].any(), f"{where}: a pass drew outside the frame's tile rows"
                assert M.pixel_nonzero(drawn).any() or r1 - r0 < frame.height, where
            model.apply(op, drawn)
        elif kind == "exchange":
            comms = groups[op["group"]]
            if op["scan"]:
                monkeypatch.setenv("CRH_EXCHANGE_SCAN_PIXELS", "1")
            else:
                monkeypatch.delenv("CRH_EXCHANGE_SCAN_PIXELS", raising=False)
            expect = model.apply(op)
            if op["fails"]:
                with pytest.raises(R.ContrastError):
                    comms[0].local_exchange([frames[j] for j in op["layers"]], frames[op["result"]])
                continue
            comms[0].local_exchange([frames[j] for j in op["layers"]], frames[op["result"]])
            if op["scan"]:
                assert_traffic(comms, expect["traffic"], where)
            else:  # the tile counts of a pass may name tiles that came out transparent: never fewer than the pixels show
                for c, e in zip(comms, expect["traffic"]):
                    assert all(a >= b for a, b in zip(c.last_peer_bytes(), e["peer_bytes"])) and c.last_traffic()[0] >= e["sent"] and c.last_traffic()[1] == e["dense"], where
        elif kind == "gather":
            groups[op["group"]][0].local_gather_slabs([frames[j] for j in op["layers"]], frames[op["result"]])
            model.apply(op)
        else:
            assert kind == "download"
            expect = model.apply(op)
            got = frames[op["frame"]].download()
            assert got.dtype == expect.dtype and got.shape == expect.shape, where
            bad = (got != expect).any(axis=2)
            assert not bad.any(), f"{where}: {int(bad.sum())} of {bad.size} pixels differ from the model, first at (row, column) {tuple(int(v) for v in np.argwhere(bad)[0])}"
