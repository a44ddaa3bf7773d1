"""Stateful fuzz of frames and the pass state they keep: random sequences of clears, crh_frame_keep_pass_state, plain and recorded passes
(cut from an episode of clip nesting and opacity groups at random draws, so that a pass may end inside an open Clip, between a Stencil
and its cover or inside a saved alpha context), instance updates, re-uploads into existing Scenes, dynamic stroke option updates, tile
slabs (crh_frame_set_tile_rows), depth uploads and loopback exchanges, over Scenes that are slices of one master batch. A host model
replays every pass with the oracle over the master batch; every download must equal it bit for bit."""
import os

import numpy as np
import pytest

from contrast_renderer_amd import scenes
from contrast_renderer_amd.renderer import Compare
from contrast_renderer_amd.renderer import RenderOperation as Op

S, CO, CL, UN, SA, SC, RE = (int(o) for o in (Op.Stencil, Op.Color, Op.Clip, Op.UnClip, Op.SaveAlphaContext, Op.ScaleAlphaContext, Op.RestoreAlphaContext))
N_FRAMES, N_SLOTS, CLIP_BITS, ALPHA_LAYERS = 3, 3, 2, 2
OP_KINDS = ("clear", "keep", "plain", "recorded", "set_instances", "tessellate", "upload", "dynamic", "tile_rows", "depth", "exchange", "download")


def leaves_state(draws):
    """Python statement of when a recorded pass leaves state with the frame: a Stencil without its cover, an open Clip, a saved alpha
    context, or a draw that relies on a level or context an earlier pass opened. draws = [(key, op, clip_depth, alpha_layer)]."""
    stencils, clips, layers = set(), [], set()
    for key, op, depth, layer in draws:
        if op == S:
            stencils.add(key)
        elif op == CO:
            stencils.discard(key)
        elif op == CL:
            stencils.discard(key)
            clips.append(key)
        elif op == UN:
            if not clips or clips[-1] != key:
                return True
            clips.pop()
        elif op == SA:
            layers.add(layer)
        elif op == RE:
            if layer not in layers:
                return True
            layers.discard(layer)
        if depth > len(clips):
            return True
    return bool(stencils or clips or layers)


def random_episode(rng, n_draw_shapes):
    """A valid episode over draw slots 0 .. n_draw_shapes - 1 (each slot one (Scene, Shape, instance)): plain Stencil + Color pairs, Clips
    nested up to the counter's depth and opacity groups up to the alpha layers, every level closed at the end. -> [(slot, op, depth, layer)]."""
    out, clips, groups = [], [], []
    for _ in range(int(rng.randint(4, 14))):
        x = int(rng.randint(0, n_draw_shapes))
        u = rng.uniform()
        depth = len(clips)
        if u < 0.2 and depth + 1 < (1 << CLIP_BITS):
            out += [(x, S, depth, 0), (x, CL, depth + 1, 0)]
            clips.append(x)
        elif u < 0.3 and clips:
            out.append((clips.pop(), UN, depth - 1, 0))
        elif u < 0.42 and len(groups) < ALPHA_LAYERS:
            out += [(x, SA, depth, len(groups)), (x, SC, depth, len(groups))]
            groups.append(x)
        elif u < 0.5 and groups:
            out.append((groups[-1], RE, depth, len(groups) - 1))
            groups.pop()
        else:
            out += [(x, S, depth, 0), (x, CO, depth, 0)]
    while clips or groups:  # (closed innermost first: a group opened inside a clip is restored before the clip goes)
        if groups and (not clips or rng.uniform() < 0.5):
            out.append((groups[-1], RE, len(clips), len(groups) - 1))
            groups.pop()
        else:
            x = clips.pop()
            out.append((x, UN, len(clips), 0))
    return out


def master_case(seed):
    """The master batch of a seed: scene_mixed, the first of its random seeds the reference can tessellate."""
    from oracle.binding import Oracle
    rng = np.random.RandomState(9100 + seed)
    n = int(rng.randint(14, 34))
    while True:
        sc = scenes.scene_mixed(n, (160, 160), seed=int(rng.randint(0, 100000)))
        if Oracle(sc["batch"]).status() == 0:
            return sc


def generate(seed, n_master):
    """The op sequence of one seed and the bookkeeping of what each frame holds (no pixels): which passes begin, continue or leave the
    frame's pass state, which frames keep state, slabs. Every random value the replay needs is in the ops."""
    rng = np.random.RandomState(5100 + seed)
    width = int(rng.randint(50, 200))
    height = int(rng.randint(64, 200))
    width += 1 if width % 16 == 0 else 0
    height += 1 if height % 16 == 0 else 0
    msaa = int(rng.choice([1, 4]))
    with_exchange = seed % 3 != 2
    depth_mode = seed % 4  # 0, 1: none; 2: tested; 3: tested and written
    formats = [0, 0, 0] if with_exchange else [int(rng.choice([0, 2])) for _ in range(N_FRAMES)]  # FORMAT_RGBA8 / FORMAT_RGBA8_ATTACHMENT
    setup = dict(width=width, height=height, msaa=msaa, formats=formats, depth_mode=depth_mode, with_exchange=with_exchange)
    frames = [dict(carry=False, started=False, episode=None, at=0, slab=None) for _ in range(N_FRAMES)]
    slots = [None] * N_SLOTS  # (a, b, instances_set)
    ops = []

    def place(n):
        t = scenes.place(width, height, rng.uniform(-10, width + 10, n), rng.uniform(-10, height + 10, n), rng.uniform(8, 0.6 * min(width, height), n))
        c = np.concatenate([rng.uniform(0, 1, (n, 3)), rng.uniform(0.2, 1, (n, 1))], axis=1).astype(np.float32)
        c[::3, 3] = 1.0
        return t.astype(np.float32), c

    def new_slice():
        a = int(rng.randint(0, n_master - 2))
        b = int(rng.randint(a + 2, min(n_master, a + 16) + 1))
        return a, b

    def drop_state(j):
        frames[j].update(carry=False, started=False, episode=None, at=0)

    def pass_into(j, op):
        f = frames[j]
        if f["carry"] and not f["started"]:
            op["start_state"] = True
            f["started"] = True
        op["carry"] = f["carry"]

    n_steps = int(rng.randint(40, 61))
    while len(ops) < n_steps:
        if all(s is None for s in slots) or rng.uniform() < 0.08:
            busy = {k for fr in frames if fr["episode"] is not None for k, _ in fr["episode_shapes"]}  # (an open episode keeps its Scenes' Shapes)
            free = [k for k in range(N_SLOTS) if k not in busy]
            if not free:
                continue
            k = free[int(rng.randint(0, len(free)))]
            a, b = new_slice() if slots[k] is None or rng.uniform() < 0.6 else slots[k][:2]  # (the same slice again: the optimistic upload)
            ops.append(dict(kind="upload", slot=k, a=a, b=b, existing=slots[k] is not None and rng.uniform() < 0.8))
            slots[k] = (a, b, False)
            continue
        kind = OP_KINDS[int(rng.choice(len(OP_KINDS), p=[0.08, 0.06, 0.2, 0.22, 0.06, 0.03, 0.0, 0.04, 0.06, 0.03, 0.07, 0.15]))]
        live = [k for k in range(N_SLOTS) if slots[k] is not None]
        j = int(rng.randint(0, N_FRAMES))
        f = frames[j]
        if kind == "clear":
            ops.append(dict(kind="clear", frame=j))
            drop_state(j)
        elif kind == "keep":
            ops.append(dict(kind="keep", frame=j))
            f["carry"] = True
        elif kind == "plain":
            if f["episode"] is not None:  # (a plain pass draws at clip depth 0: not inside an open episode)
                continue
            k = live[int(rng.randint(0, len(live)))]
            a, b, inst = slots[k]
            op = dict(kind="plain", frame=j, slot=k)
            if not inst or rng.uniform() < 0.5:
                op["instances"] = place(b - a)
                slots[k] = (a, b, True)
            pass_into(j, op)
            ops.append(op)
        elif kind == "recorded":
            if f["episode"] is None:
                picks = [live[int(rng.randint(0, len(live)))] for _ in range(int(rng.randint(1, 4)))]  # the Scenes the episode draws from
                draw_shapes = []
                for k in picks:
                    a, b, _ = slots[k]
                    for _ in range(int(rng.randint(2, 6))):
                        draw_shapes.append((k, int(rng.randint(0, b - a))))
                f["episode"], f["at"], f["episode_shapes"] = random_episode(rng, len(draw_shapes)), 0, draw_shapes
                f["episode_instances"] = place(len(draw_shapes))
            epi = f["episode"]
            end = int(rng.randint(f["at"] + 1, len(epi) + 1)) if rng.uniform() < 0.6 else len(epi)
            chunk = epi[f["at"]:end]
            # the chunk's draws are (slot, local shape, pass instance, op, depth, layer); slices may have been re-uploaded since the episode began:
            # a draw whose Scene no longer holds that Shape index is drawn from shape 0 of it
            draws = []
            for x, o, depth, layer in chunk:
                k, s = f["episode_shapes"][x]
                a, b, _ = slots[k]
                draws.append((k, min(s, b - a - 1), x, o, depth, layer))
            t, c = f["episode_instances"]
            op = dict(kind="recorded", frame=j, draws=draws, transforms=t, colors=c, episode_start=f["at"] == 0)
            op["leaves"] = leaves_state([((k, s, x), o, depth, layer) for k, s, x, o, depth, layer in draws])
            spans = len(set(d[0] for d in draws)) > 1
            if spans or op["leaves"]:
                f["carry"] = True  # (RenderPass.submit keeps the state of a pass over several Scene objects; a pass that leaves state keeps it by itself)
            pass_into(j, op)
            f["at"] = end
            if end == len(epi):
                f["episode"] = None
            op["closed"] = f["episode"] is None
            ops.append(op)
        elif kind == "set_instances":
            k = live[int(rng.randint(0, len(live)))]
            a, b, _ = slots[k]
            ops.append(dict(kind="set_instances", slot=k, instances=place(b - a)))
            slots[k] = (a, b, True)
        elif kind == "tessellate":
            ops.append(dict(kind="tessellate", slot=live[int(rng.randint(0, len(live)))]))
        elif kind == "dynamic":
            if any(fr["carry"] for fr in frames):  # (the model draws a kept state's passes again with the options of today)
                continue
            k = live[int(rng.randint(0, len(live)))]
            a, b, _ = slots[k]
            ops.append(dict(kind="dynamic", shape=int(rng.randint(a, b)), pick=int(rng.randint(0, 1 << 30)), join=int(rng.randint(0, 3)),
                            caps=[int(v) for v in rng.randint(0, 7, 2)], dash=sorted(float(v) for v in rng.uniform(0.3, 3.0, 2)), phase=float(rng.uniform(-1, 1))))
        elif kind == "tile_rows":
            if j == 2:  # (the frame the exchanges write keeps its whole rows)
                continue
            if f["slab"] is None or rng.uniform() < 0.3:
                r0 = 16 * int(rng.randint(0, (height - 1) // 16 + 1))
                r1 = min(height, 16 * int(rng.randint(r0 // 16 + 1, (height - 1) // 16 + 2)))
            else:
                r0, r1 = 0, height
            ops.append(dict(kind="tile_rows", frame=j, rows=(r0, r1), after_carry=f["carry"] and f["started"]))
            drop_state(j)
            f["slab"] = None if (r0, r1) == (0, height) else (r0, r1)
        elif kind == "depth":
            if depth_mode < 2 or f["carry"]:
                continue
            ops.append(dict(kind="depth", frame=j, depth=rng.choice([0.2, 0.6, 0.95, 1.0], size=(height, width)).astype(np.float32)))
        elif kind == "exchange":
            if not with_exchange or frames[2]["episode"] is not None:  # (into a frame that keeps state only when every pass closed its state)
                continue
            ops.append(dict(kind="exchange"))
            frames[2]["started"] = False  # (the planes start again from the exchanged image: carry_recolor, with zero counters)
        else:
            ops.append(dict(kind="download", frame=j))
    ops += [dict(kind="download", frame=j) for j in range(N_FRAMES)]
    return setup, ops


def _seeds():
    return range(int(os.environ.get("CRH_FUZZ_LIFECYCLE_SEEDS", "12")))


# The fuzz under the default and under the pins of the paths it crosses: the triangle formulation, the exact tile lists (no places kept),
# the upload that tessellates without the optimistic capacity, the two-pass tessellation. (Fewer seeds each: the suite's time budget.)
LIFECYCLE_PINS = [None, ("CRH_TRIANGLE_PASS", "1"), ("CRH_NO_DIRECT_LISTS", "1"), ("CRH_NO_OPTIMISTIC_UPLOAD", "1"), ("CRH_TESS_TWO_PASS", "1")]


def _pinned_runs():
    per_pin = int(os.environ.get("CRH_FUZZ_LIFECYCLE_PIN_SEEDS", "6"))
    return [(pin, seed) for pin in LIFECYCLE_PINS for seed in (_seeds() if pin is None else range(per_pin))]


def test_the_lifecycle_generator_reaches_every_op_and_leaves_state(oracle_lib):
    """CPU only: the op generator and its bookkeeping over every seed of the GPU fuzz — every op kind occurs, passes end with state left
    over, a set_tile_rows follows a frame that keeps state, exchanges meet frames that keep state. Keeps the fuzz from degenerating."""
    kinds, leftover, after_carry, exchange_into_carry, spans, starts = set(), 0, 0, 0, 0, 0
    for seed in _seeds():
        sc = master_case(seed)
        setup, ops = generate(seed, sc["batch"].n_shapes)
        assert 40 <= len(ops) and setup["width"] % 16 and setup["height"] % 16
        carry2 = False
        for op in ops:
            kinds.add(op["kind"])
            if op["kind"] == "recorded":
                leftover += int(not op["closed"])
                spans += int(len(set(d[0] for d in op["draws"])) > 1)
                starts += int(op.get("start_state", False))
                carry2 = carry2 or (op["frame"] == 2 and op["carry"])
            after_carry += int(op["kind"] == "tile_rows" and op["after_carry"])
            if op["kind"] == "clear" and op["frame"] == 2:
                carry2 = False
            exchange_into_carry += int(op["kind"] == "exchange" and carry2)
    assert kinds == set(OP_KINDS), set(OP_KINDS) - kinds
    assert leftover >= 10 and spans >= 5 and starts >= 5, (leftover, spans, starts)
    assert after_carry >= 2 and exchange_into_carry >= 1, (after_carry, exchange_into_carry)


def test_python_statement_of_leftover_state_matches_the_library(oracle_lib):
    """leaves_state (the fuzz's own reading of its draws) against crh_debug_pass_leaves_state, over every recorded pass the generator makes."""
    import ctypes as C
    from contrast_renderer_amd import _ffi
    lib = _ffi.load_library()
    lib.crh_debug_pass_leaves_state.restype = C.c_int
    lib.crh_debug_pass_leaves_state.argtypes = [C.c_void_p, C.c_uint32]
    checked = 0
    for seed in _seeds():
        setup, ops = generate(seed, master_case(seed)["batch"].n_shapes)
        for op in ops:
            if op["kind"] != "recorded" or len(set(d[0] for d in op["draws"])) > 1:
                continue
            table = np.array([d[1:] for d in op["draws"]], dtype=np.uint32).reshape(-1, 5)
            assert lib.crh_debug_pass_leaves_state(table.ctypes.data, len(table)) == int(op["leaves"]), op["draws"]
            checked += 1
    assert checked >= 20


class Model:
    """What each frame must hold, from the oracle over the master batch."""

    def __init__(self, setup, batch, render_pass, Oracle):
        self.s, self.batch, self.render_pass, self.Oracle = setup, batch, render_pass, Oracle
        self.oracle = Oracle(batch)
        w, h, msaa = setup["width"], setup["height"], setup["msaa"]
        self.depth = setup["depth_mode"] >= 2
        self.image = [np.zeros((h, w, 4), np.uint8) for _ in range(N_FRAMES)]
        self.z = [np.ones((h, w, msaa), np.float32) if self.depth else None for _ in range(N_FRAMES)]
        self.cleared = [True] * N_FRAMES
        self.slab = [None] * N_FRAMES
        self.kept = [None] * N_FRAMES  # a frame's kept state: dict(base, zbase, draws, transforms, colors)

    def state(self):
        less = int(Compare.Less)
        return dict(depth_compare=less, depth_write=1) if self.s["depth_mode"] == 3 else (dict(depth_compare=less) if self.s["depth_mode"] == 2 else {})

    def draw(self, j, draws, t, c, op):
        """draws: oracle draws (master shape, instance, op, depth, layer) with instances t / c."""
        w, h, msaa = self.s["width"], self.s["height"], self.s["msaa"]
        if op.get("start_state"):
            self.kept[j] = dict(base=None if self.cleared[j] else self.image[j].copy(), zbase=None if self.z[j] is None else self.z[j].copy(), draws=[], t=[], c=[])
        if op["carry"]:
            k = self.kept[j]
            off = sum(len(x) for x in k["t"])
            k["draws"] += [(s, i + off, o, d, a) for s, i, o, d, a in draws]
            k["t"].append(t), k["c"].append(c)
            image, z = self.render_pass(self.oracle, w, h, msaa, 4, CLIP_BITS, ALPHA_LAYERS, np.concatenate(k["t"]), np.concatenate(k["c"]), k["draws"],
                                        depth=k["zbase"], load=k["base"], attachment8=self.s["formats"][j] == 2, **self.state())
        else:
            image, z = self.render_pass(self.oracle, w, h, msaa, 4, CLIP_BITS, ALPHA_LAYERS, t, c, draws, depth=self.z[j],
                                        load=None if self.cleared[j] else self.image[j], attachment8=self.s["formats"][j] == 2, **self.state())
        if self.slab[j] is not None:  # rows outside the slab: transparent, their depth untouched
            r0, r1 = self.slab[j]
            image[:r0] = 0
            image[r1:] = 0
            if z is not None:
                z[:r0] = self.z[j][:r0]
                z[r1:] = self.z[j][r1:]
        self.image[j], self.z[j], self.cleared[j] = image, z, False


@pytest.mark.gpu
@pytest.mark.parametrize("pin,seed", _pinned_runs(), ids=[f"{pin[0] if pin else 'default'}-{seed}" for pin, seed in _pinned_runs()])
def test_random_frame_lifecycles_against_a_host_model(pin, seed, oracle_lib, monkeypatch):
    """The op sequence of generate(seed) on the GPU, every download against the host model; under a pin, the passes took the path it names
    (crh_debug_frame_last_pass; CRH_TESS_TWO_PASS: the tessellation's timing marks). CRH_NO_OPTIMISTIC_UPLOAD leaves no mark of its own:
    that run checks pixels."""
    import torch
    assert torch.cuda.is_available()
    from contrast_renderer_amd import Cap, DashInterval, DynamicStrokeOptions, Join, distributed
    from contrast_renderer_amd import renderer as R
    from oracle.binding import Oracle, render_pass
    from test_gpu_fuzz import _no_path_pins, last_pass, tess_marks
    _no_path_pins(monkeypatch)
    if pin:
        monkeypatch.setenv(*pin)  # (before the Renderer and the Scenes: pins are read per pass and per upload)
    taps = []
    sc = master_case(seed)
    batch = sc["batch"]
    setup, ops = generate(seed, batch.n_shapes)
    w, h, msaa = setup["width"], setup["height"], setup["msaa"]
    model = Model(setup, batch, render_pass, Oracle)
    st = model.state()
    r = R.Renderer(R.Configuration(msaa, CLIP_BITS, 4, ALPHA_LAYERS, depth_compare=st.get("depth_compare", 0), depth_write_enabled=bool(st.get("depth_write", 0))), device=0)
    frames = [R.Frame(r, w, h, setup["formats"][j]) for j in range(N_FRAMES)]
    for f in frames:
        f.clear()
    comms = None
    if setup["with_exchange"]:
        comms = [R.Comm(r, 0, 2)]
        comms.append(R.Comm(r, 1, 2, rank0=comms[0]))
    slots = [None] * N_SLOTS  # dict(scene, a, b, t, c)
    lib = r.lib
    import ctypes as C
    lib.crh_debug_pass_leaves_state.restype = C.c_int
    lib.crh_debug_pass_leaves_state.argtypes = [C.c_void_p, C.c_uint32]
    for step, op in enumerate(ops):
        kind = op["kind"]
        where = f"seed {seed} step {step} ({kind})"
        if kind == "upload":
            old = slots[op["slot"]]
            scene = R.Scene(r, batch.slice_shapes(op["a"], op["b"]), existing=old["scene"] if (old and op["existing"]) else None)
            assert scene.status() == 0, where
            slots[op["slot"]] = dict(scene=scene, a=op["a"], b=op["b"], t=None, c=None)
        elif kind == "clear":
            frames[op["frame"]].clear()
            j = op["frame"]
            model.image[j] = np.zeros_like(model.image[j])
            model.cleared[j], model.kept[j] = True, None
            if model.z[j] is not None:
                model.z[j] = np.ones_like(model.z[j])
        elif kind == "keep":
            frames[op["frame"]].keep_pass_state()
        elif kind == "plain":
            s = slots[op["slot"]]
            if "instances" in op:
                s["t"], s["c"] = op["instances"]
                s["scene"].render(frames[op["frame"]], s["t"], s["c"])
            else:
                s["scene"].render(frames[op["frame"]])
            n = s["b"] - s["a"]
            draws = [d for i in range(n) for d in ((s["a"] + i, i, S, 0, 0), (s["a"] + i, i, CO, 0, 0))]
            model.draw(op["frame"], draws, s["t"], s["c"], op)
            taps.append(last_pass(frames[op["frame"]]))
        elif kind == "recorded":
            p = R.RenderPass(r, frames[op["frame"]])
            for t, c in zip(op["transforms"], op["colors"]):
                p.push_instance(t, c)
            for k, s_local, x, o, depth, layer in op["draws"]:
                p.set_clip_depth(depth)
                p.set_alpha_layer(layer)
                p.render(slots[k]["scene"], [x], o, shape_index=s_local)
            if len(set(d[0] for d in op["draws"])) == 1:
                table = np.array([d[1:] for d in op["draws"]], dtype=np.uint32).reshape(-1, 5)
                assert lib.crh_debug_pass_leaves_state(table.ctypes.data, len(table)) == int(op["leaves"]), where
            p.submit()
            draws = [(slots[k]["a"] + s_local, x, o, depth, layer) for k, s_local, x, o, depth, layer in op["draws"]]
            model.draw(op["frame"], draws, op["transforms"], op["colors"], op)
            taps.append(last_pass(frames[op["frame"]]))
        elif kind == "set_instances":
            s = slots[op["slot"]]
            s["t"], s["c"] = op["instances"]
            s["scene"].set_instances(s["t"], s["c"])
        elif kind == "tessellate":
            slots[op["slot"]]["scene"].tessellate()
        elif kind == "dynamic":
            shape = op["shape"]
            d0, d1 = int(batch.shape_dynamic_begin[shape]), int(batch.shape_dynamic_begin[shape + 1])
            if d1 == d0:
                continue
            group = op["pick"] % (d1 - d0)
            caps = [Cap(v) for v in op["caps"]]
            if batch.dynamic_stroke_options[d0 + group].dashed:  # (a dashed group stays dashed, a solid one solid: the same tessellation)
                new = DynamicStrokeOptions.Dashed(Join(op["join"]), [DashInterval(op["dash"][0], op["dash"][1] + 0.2, caps[0], caps[1])], op["phase"])
            else:
                new = DynamicStrokeOptions.Solid(Join(op["join"]), caps[0], caps[1])
            batch.dynamic_stroke_options[d0 + group] = new.to_c()
            model.oracle = Oracle(batch)
            for s in slots:  # every Scene that holds the Shape mirrors the master batch
                if s is not None and s["a"] <= shape < s["b"]:
                    s["scene"].set_dynamic_stroke_options(shape - s["a"], group, new)
        elif kind == "tile_rows":
            j = op["frame"]
            frames[j].set_tile_rows(*op["rows"])
            model.image[j] = np.zeros_like(model.image[j])
            model.cleared[j], model.kept[j] = True, None
            model.slab[j] = None if tuple(op["rows"]) == (0, h) else tuple(op["rows"])
        elif kind == "depth":
            j = op["frame"]
            frames[j].upload_depth(op["depth"])
            model.z[j] = np.repeat(op["depth"][:, :, None], msaa, axis=2)
        elif kind == "exchange":
            comms[0].local_exchange(frames[:2], frames[2])
            model.image[2] = distributed.composite_over_reference(np.stack(model.image[:2]))
            model.cleared[2], model.kept[2] = False, None  # (a frame that keeps state starts its planes again from this image at its next pass)
        else:
            j = op["frame"]
            image = frames[j].download()
            assert np.array_equal(image, model.image[j]), f"{where}: frame {j}, {(image != model.image[j]).any(axis=2).sum()} pixels differ"
    assert taps and all(t["raster"] != "none" for t in taps), taps
    name = pin[0] if pin else None
    if name == "CRH_TRIANGLE_PASS":
        assert all(t["formulation"] == 2 and t["raster"] in ("tile", "ops") for t in taps), taps
    elif name == "CRH_NO_DIRECT_LISTS":
        assert not any(t["direct"] for t in taps), taps
    elif name == "CRH_TESS_TWO_PASS":
        kernels = tess_marks(r, next(s for s in slots if s is not None)["scene"])
        assert "tess_emit" in kernels and "tess_fused" not in kernels, kernels


@pytest.mark.gpu
@pytest.mark.parametrize("msaa", [1, 4])
@pytest.mark.parametrize("rows", ["whole", "slab"])
def test_set_tile_rows_drops_the_pass_state_of_the_frame(msaa, rows, oracle_lib):
    """crh_frame_set_tile_rows is a LoadOp::Clear of the pixels, the stencil attachment and the alpha layers: on a frame that keeps its pass
    state, with the planes valid and a Clip still open, the plain pass after it is the oracle's image of that pass alone — no colour from
    before the call, no confinement by the open Clip — and with a slab (16, 48) every row outside it is transparent."""
    import torch
    assert torch.cuda.is_available()
    from contrast_renderer_amd import renderer as R
    from oracle.binding import Oracle, render_pass
    sc = scenes.scene_mixed(10, (150, 120), seed=31)
    o = Oracle(sc["batch"])
    assert o.status() == 0
    w, h, n = 150, 120, sc["batch"].n_shapes
    r = R.Renderer(R.Configuration(msaa, CLIP_BITS, 4, ALPHA_LAYERS), device=0)
    scene = R.Scene(r, sc["batch"])
    frame = R.Frame(r, w, h)
    rng = np.random.RandomState(3)
    t_before = scenes.place(w, h, rng.uniform(0, w, n), rng.uniform(0, h, n), rng.uniform(30, 70, n)).astype(np.float32)
    c_before = np.concatenate([rng.uniform(0, 1, (n, 3)), np.ones((n, 1))], axis=1).astype(np.float32)
    t_after = scenes.place(w, h, rng.uniform(0, w, n), rng.uniform(0, h, n), rng.uniform(10, 40, n)).astype(np.float32)
    c_after = np.concatenate([rng.uniform(0, 1, (n, 3)), rng.uniform(0.3, 1, (n, 1))], axis=1).astype(np.float32)
    t_before[0] = scenes.place(w, h, np.array([w / 2]), np.array([h / 2]), np.array([25.0]))[0]  # the clip: a small Shape in the middle
    frame.clear()
    frame.keep_pass_state()
    opened = [(0, 0, S, 0, 0), (0, 0, CL, 1, 0)] + [d for i in range(1, n // 2) for d in ((i, i, S, 1, 0), (i, i, CO, 1, 0))]
    scene.render_draws(frame, t_before, c_before, opened)  # ends inside the open Clip
    scene.render_draws(frame, t_before, c_before, [d for i in range(n // 2, n) for d in ((i, i, S, 1, 0), (i, i, CO, 1, 0))])  # the planes are valid now
    assert frame.download()[..., 3].any()
    r0, r1 = (0, h) if rows == "whole" else (16, 48)
    frame.set_tile_rows(r0, r1)
    scene.render(frame, t_after, c_after)
    image = frame.download()
    plain = [d for i in range(n) for d in ((i, i, S, 0, 0), (i, i, CO, 0, 0))]
    expect, _ = render_pass(o, w, h, msaa, 4, CLIP_BITS, ALPHA_LAYERS, t_after, c_after, plain)
    expect[:r0] = 0
    expect[r1:] = 0
    assert expect[r0:r1, ..., 3].any()
    assert np.array_equal(image, expect), f"{(image != expect).any(axis=2).sum()} pixels differ"
