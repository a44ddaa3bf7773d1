"""Randomised parity sweep of the HIP path against the oracle: scenes with every segment type, fills and strokes, random frame sizes
(not multiples of the tile), sample counts, winding rules, plain or perspective instance transforms, depth / cull states and recorded
passes with clip nesting — each case small enough for the oracle to render in a fraction of a second. Bit for bit."""
import math

import numpy as np
import pytest

from contrast_renderer_amd import scenes, utils
from contrast_renderer_amd.renderer import Compare, Cull
from contrast_renderer_amd.renderer import RenderOperation as Op


def random_case(seed):
    rng = np.random.RandomState(1000 + seed)
    width, height = int(rng.randint(40, 300)), int(rng.randint(40, 300))
    msaa = int(rng.choice([1, 4]))
    winding_bits = int(rng.choice([1, 2, 4]))
    n_shapes = int(rng.randint(3, 40))
    base = scenes.scene_mixed(n_shapes, (max(width, 96), max(height, 96)), seed=seed)
    batch, colors = base["batch"], base["colors"]
    n = batch.n_shapes
    kind = seed % 6
    if kind == 0 or kind == 4:  # plain instances, placed over the (smaller) frame so that shapes hang over every border
        t = scenes.place(width, height, rng.uniform(-10, width + 10, n), rng.uniform(-10, height + 10, n), rng.uniform(8, 0.5 * min(width, height), n))
    elif kind == 5:  # extreme placements: tiny and enormous scales, centres far outside the frame (slivers, clamped boxes, huge coordinates)
        t = scenes.place(width, height, rng.uniform(-3 * width, 4 * width, n), rng.uniform(-3 * height, 4 * height, n),
                         np.exp(rng.uniform(math.log(0.05), math.log(40.0 * max(width, height)), n)))
    else:  # perspective: tilted decals at random depths, some reaching through the near plane
        projection = utils.perspective_projection(math.pi * 0.5, width / height, 1.0, 100.0)
        t = np.stack([utils.matrix_multiplication(projection, utils.matrix_multiplication(
            utils.translation_matrix(rng.uniform(-2, 2), rng.uniform(-2, 2), rng.uniform(0.8, 6.0)),
            utils.rotation_matrix(rng.uniform(-1.4, 1.4), (math.cos(i * 1.7), math.sin(i * 1.7), 0.0)))) for i in range(n)])
    state = {}
    if kind == 2:
        state = dict(depth_compare=int(rng.choice([Compare.Less, Compare.LessEqual, Compare.Greater, Compare.NotEqual])), depth_write=int(rng.randint(0, 2)),
                     cull_mode=int(rng.choice([Cull.Disabled, Cull.Back])))
    draws = []
    if kind == 3:  # a recorded pass: the first shape clips the second half of the shapes; instancing reuses shape 0
        draws += [(0, 0, Op.Stencil, 0, 0), (0, 0, Op.Clip, 1, 0)]
        for i in range(n // 2, n):
            draws += [(i, i, Op.Stencil, 1, 0), (i, i, Op.Color, 1, 0)]
        draws += [(0, 0, Op.UnClip, 0, 0)]
        for i in range(1, n // 2):
            draws += [(i, i, Op.Stencil, 0, 0), (i, i, Op.Color, 0, 0)]
        draws += [(0, n - 1, Op.Stencil, 0, 0), (0, n - 1, Op.Color, 0, 0)]
    elif kind == 4:  # an opacity group (Save / Scale / content / Restore) over a background, twice nested
        draws += [(0, 0, Op.Stencil, 0, 0), (0, 0, Op.Color, 0, 0), (1, 1, Op.SaveAlphaContext, 0, 0), (1, 1, Op.ScaleAlphaContext, 0, 0)]
        for i in range(2, n // 2):
            draws += [(i, i, Op.Stencil, 0, 0), (i, i, Op.Color, 0, 0)]
        draws += [(2, 2, Op.SaveAlphaContext, 0, 1), (2, 2, Op.ScaleAlphaContext, 0, 1)]
        for i in range(n // 2, n):
            draws += [(i, i, Op.Stencil, 0, 0), (i, i, Op.Color, 0, 0)]
        draws += [(2, 2, Op.RestoreAlphaContext, 0, 1), (1, 1, Op.RestoreAlphaContext, 0, 0)]
    else:
        for i in range(n):
            draws += [(i, i, Op.Stencil, 0, 0), (i, i, Op.Color, 0, 0)]
    depth = None
    if state.get("depth_compare", 0) or state.get("depth_write", 0):
        depth = rng.choice([0.2, 0.6, 0.95, 1.0], size=(height, width)).astype(np.float32)
    return dict(width=width, height=height, msaa=msaa, winding_bits=winding_bits, batch=batch, transforms=t.astype(np.float32), colors=colors, draws=draws,
                state=state, depth=depth)


@pytest.mark.gpu
@pytest.mark.parametrize("seed", range(int(__import__("os").environ.get("CRH_FUZZ_SEEDS", "48"))))
def test_random_scene_matches_the_oracle(seed, oracle_lib):
    import torch
    assert torch.cuda.is_available()
    check_random_case(seed)


def check_random_case(seed, marks=False):
    """random_case(seed) drawn once and compared with the oracle -> dict(taps=[what the pass ran (last_pass)], kernels=the tessellation's
    timing marks when `marks`), or None for a scene the reference cannot tessellate."""
    from contrast_renderer_amd import renderer as R
    from oracle.binding import Oracle, render_pass
    c = random_case(seed)
    o = Oracle(c["batch"])
    config = R.Configuration(msaa_sample_count=c["msaa"], clip_nesting_counter_bits=2, winding_counter_bits=c["winding_bits"], alpha_layer_count=2,
                             cull_mode=c["state"].get("cull_mode", 0), depth_compare=c["state"].get("depth_compare", 0),
                             depth_write_enabled=bool(c["state"].get("depth_write", 0)))
    r = R.Renderer(config, device=0)
    scene = R.Scene(r, c["batch"])
    assert scene.status() == o.status()  # a scene the reference cannot tessellate (fill.rs:174,178 panics) fails the same way
    if o.status() != 0:
        return None
    expect, expect_depth = render_pass_rect(o, c, render_pass)
    frame = R.Frame(r, c["width"], c["height"])
    frame.clear()
    if c["depth"] is not None:
        frame.upload_depth(c["depth"])
    scene.render_draws(frame, c["transforms"], c["colors"], c["draws"])
    image = frame.download()
    assert np.array_equal(image, expect), f"seed {seed}: {(image != expect).any(axis=2).sum()} pixels differ"
    if c["depth"] is not None:
        assert np.array_equal(frame.download_depth(), expect_depth)
    return dict(taps=[last_pass(frame)], kernels=tess_marks(r, scene) if marks else None)


@pytest.mark.gpu
@pytest.mark.parametrize("seed", range(int(__import__("os").environ.get("CRH_FUZZ_SPLIT_SEEDS", "24"))))
def test_a_random_pass_cut_into_pieces_at_random_draws_gives_the_same_frame(seed, oracle_lib):
    """The recorded pass of random_case(seed) submitted as two to five passes cut at random draws (between a Stencil and its cover, inside an
    open clip, inside an opacity group): with the pass state kept on the frame (crh_frame_keep_pass_state: the reference's caller-owned stencil
    attachment, alpha layers and f32 colour, renderer.rs:148-158, 257-266) the frame is the single pass's, bit for bit."""
    import torch
    assert torch.cuda.is_available()
    from contrast_renderer_amd import renderer as R
    from oracle.binding import Oracle, render_pass
    c = random_case(seed)
    o = Oracle(c["batch"])
    if o.status() != 0:
        pytest.skip("the reference cannot tessellate this scene (covered by test_random_scene_matches_the_oracle)")
    rng = np.random.RandomState(7000 + seed)
    config = R.Configuration(msaa_sample_count=c["msaa"], clip_nesting_counter_bits=2, winding_counter_bits=c["winding_bits"], alpha_layer_count=2,
                             cull_mode=c["state"].get("cull_mode", 0), depth_compare=c["state"].get("depth_compare", 0),
                             depth_write_enabled=bool(c["state"].get("depth_write", 0)))
    r = R.Renderer(config, device=0)
    scene = R.Scene(r, c["batch"])
    expect, expect_depth = render_pass_rect(o, c, render_pass)
    draws = c["draws"]
    pieces = min(len(draws), int(rng.randint(2, 6)))
    cuts = sorted(rng.choice(np.arange(1, len(draws)), size=pieces - 1, replace=False).tolist()) if len(draws) > 1 else []
    bounds = [0] + cuts + [len(draws)]
    frame = R.Frame(r, c["width"], c["height"])
    for round_ in range(2):  # the second round after a clear: the state of the first must be gone
        frame.clear()
        if c["depth"] is not None:
            frame.upload_depth(c["depth"])
        frame.keep_pass_state()
        for a, b in zip(bounds[:-1], bounds[1:]):
            scene.render_draws(frame, c["transforms"], c["colors"], draws[a:b])
        image = frame.download()
        assert np.array_equal(image, expect), f"seed {seed} cuts {cuts} round {round_}: {(image != expect).any(axis=2).sum()} pixels differ"
        if c["depth"] is not None:
            assert np.array_equal(frame.download_depth(), expect_depth)


def render_pass_rect(o, c, render_pass):
    """oracle.binding.render_pass takes (width, height); kept in one place so that the argument order cannot drift from the GPU call."""
    return render_pass(o, c["width"], c["height"], c["msaa"], c["winding_bits"], 2, 2, c["transforms"], c["colors"], [tuple(int(v) for v in d) for d in c["draws"]],
                       depth=c["depth"], **c["state"])


def random_paths(n_shapes, seed):
    """Unstructured geometry: random control points (self-intersecting outlines, loops, cusps, coincident and collinear points, weights
    from 0.2 to 5), one to three paths per Shape, filled or stroked with random widths / offsets / joins / caps / approximations."""
    from contrast_renderer_amd import Cap, CurveApproximation, DashInterval, DynamicStrokeOptions, Join, Path, StrokeOptions
    rng = np.random.RandomState(seed)
    caps = list(Cap)
    shapes = []
    for s in range(n_shapes):
        paths, dynamic = [], []
        for _ in range(rng.randint(1, 4)):
            scale = float(np.exp(rng.uniform(math.log(0.05), math.log(3.0))))

            def pt():
                if rng.uniform() < 0.08 and paths:  # reuse an earlier point: coincident vertices
                    return paths[-1].start
                return (float(np.float32(rng.normal(0, scale))), float(np.float32(rng.normal(0, scale))))
            pen = pt()
            p = Path(start=pen)
            for _ in range(rng.randint(1, 10)):
                kind = rng.randint(0, 5)
                end = pen if rng.uniform() < 0.05 else pt()
                if kind == 0:
                    p.push_line(end)
                elif kind == 1:
                    p.push_integral_quadratic_curve(pt(), end)
                elif kind == 2:
                    p.push_integral_cubic_curve(pt(), pt(), end)
                elif kind == 3:
                    p.push_rational_quadratic_curve(float(np.exp(rng.uniform(-1.6, 1.6))), pt(), end)
                else:
                    p.push_rational_cubic_curve(np.exp(rng.uniform(-1.6, 1.6, 4)), pt(), pt(), end)
                pen = end
            if rng.uniform() < 0.5:
                approx = CurveApproximation.UniformTangentAngle(float(rng.uniform(0.05, 0.8))) if rng.uniform() < 0.5 else CurveApproximation.UniformlySpacedParameters(int(rng.randint(1, 12)))
                p.stroke_options = StrokeOptions(float(rng.uniform(0.001, 0.5)), float(rng.uniform(-0.5, 0.5)), float(rng.uniform(1.0, 8.0)), bool(rng.randint(0, 2)),
                                                 len(dynamic), approx)
                join = (Join.Miter, Join.Bevel, Join.Round)[rng.randint(0, 3)]
                if rng.uniform() < 0.5:
                    dynamic.append(DynamicStrokeOptions.Solid(join, caps[rng.randint(0, len(caps))], caps[rng.randint(0, len(caps))]))
                else:
                    a, b = sorted(rng.uniform(0.0, 4.0, 2))
                    dynamic.append(DynamicStrokeOptions.Dashed(join, [DashInterval(float(a), float(b), caps[rng.randint(0, len(caps))], caps[rng.randint(0, len(caps))])],
                                                               float(rng.uniform(0.0, 2.0))))
            paths.append(p)
        shapes.append((dynamic, paths))
    return shapes


@pytest.mark.gpu
@pytest.mark.parametrize("seed", range(int(__import__("os").environ.get("CRH_FUZZ_PATH_SEEDS", "4"))))
def test_random_paths_tessellate_to_the_same_bytes_or_fail_the_same_way(seed, oracle_lib):
    import torch
    assert torch.cuda.is_available()
    from contrast_renderer_amd import batch_from_shapes
    from contrast_renderer_amd import renderer as R
    from oracle.binding import Oracle
    shapes = random_paths(1500, 77 + seed)
    batch = batch_from_shapes(shapes)
    oracle = Oracle(batch, 8)
    status = [oracle.shape_status(s) for s in range(len(shapes))]
    good = [s for s in range(len(shapes)) if status[s] == 0]
    assert len(good) > 0.5 * len(shapes)
    r = R.Renderer(R.Configuration(1, 4, 4), device=0)
    clean = batch_from_shapes([shapes[s] for s in good])
    scene = R.Scene(r, clean)
    assert scene.status() == 0
    layout, vb, ib = scene.all_shapes()
    olayout, ovb, oib = Oracle(clean, 8).all_shapes()
    assert np.array_equal(layout, olayout) and np.array_equal(ib, oib)
    assert np.array_equal(vb, ovb), f"{np.flatnonzero(vb != ovb).size} vertex bytes differ, first at {np.flatnonzero(vb != ovb)[0]}"
    assert vb.size > 1_000_000
    for s in [s for s in range(len(shapes)) if status[s] != 0][:8]:  # what the reference cannot tessellate fails with the same code
        assert R.Scene(r, batch.slice_shapes(s, s + 1)).status() == status[s]
    # and the pixels of a frame over them
    n = clean.n_shapes
    rng = np.random.RandomState(seed)
    t = scenes.place(256, 256, rng.uniform(0, 256, n), rng.uniform(0, 256, n), rng.uniform(5, 60, n))
    c = np.concatenate([rng.uniform(0, 1, (n, 3)), rng.uniform(0.2, 1, (n, 1))], axis=1).astype(np.float32)
    frame = R.Frame(r, 256, 256)
    frame.clear()
    scene.render(frame, t, c)
    image = frame.download()
    expect = Oracle(clean, 8).render(256, 256, 1, 4, t, c)
    assert np.array_equal(image, expect), f"{(image != expect).any(axis=2).sum()} pixels differ"


@pytest.mark.gpu
def test_two_renderers_and_reused_scenes_interleaved(oracle_lib):
    """Two Renderers on the same GPU (each with its own streams) driven alternately without synchronisation in between, each re-uploading
    scenes of changing size into the same Scene object (`existing_shape`, renderer.rs:216-221) and rendering into two frames of its own:
    every download matches the oracle."""
    import torch
    assert torch.cuda.is_available()
    from contrast_renderer_amd import renderer as R
    from oracle.binding import Oracle
    renderers = [R.Renderer(R.Configuration(1, 4, 4), device=0), R.Renderer(R.Configuration(4, 2, 4), device=0)]
    frames = [[R.Frame(r, 200 + 56 * k, 150 + 40 * k) for k in range(2)] for r in renderers]
    held = [None, None]
    pending = []
    for step in range(12):
        which = step % 2
        r = renderers[which]
        sc = scenes.scene_mixed(4 + (step * 7) % 23, (256, 256), seed=100 + step)
        if Oracle(sc["batch"]).status() != 0:
            continue
        held[which] = R.Scene(r, sc["batch"], existing=held[which])
        frame = frames[which][(step // 2) % 2]
        frame.clear()
        held[which].render(frame, sc["transforms"], sc["colors"])
        pending = [q for q in pending if q[0] is not frame] + [(frame, sc, r.config.msaa_sample_count)]  # the last render into each frame
    checked = 0
    for f, s, msaa in pending:
        expect = Oracle(s["batch"]).render(f.width, f.height, msaa, 4, s["transforms"], s["colors"])
        assert np.array_equal(f.download(), expect)
        checked += 1
    assert checked == 4


@pytest.mark.gpu
def test_objects_may_be_destroyed_in_any_order(oracle_lib):
    """Host bindings finalise in any order (a garbage collector, a scope exit): a Renderer destroyed before its Scenes and Frames orphans
    them, and a Scene destroyed while a Frame still refers to it (deferred tile-list check) settles that Frame first."""
    import torch
    assert torch.cuda.is_available()
    from contrast_renderer_amd import renderer as R
    from oracle.binding import Oracle
    sc = scenes.scene_mixed(9, (128, 128), seed=1)
    expect = Oracle(sc["batch"]).render(128, 128, 1, 4, sc["transforms"], sc["colors"])
    for order in ("renderer_first", "scene_first", "frame_first"):
        r = R.Renderer(R.Configuration(1, 4, 4), device=0)
        scene = R.Scene(r, sc["batch"])
        frame = R.Frame(r, 128, 128)
        frame.clear()
        scene.render(frame, sc["transforms"], sc["colors"])
        lib = r.lib
        if order == "renderer_first":
            lib.crh_renderer_destroy(r.handle)
            r.handle = None
            lib.crh_scene_destroy(scene.handle)
            scene.handle = None
            lib.crh_frame_destroy(frame.handle)
            frame.handle = None
        elif order == "scene_first":
            lib.crh_scene_destroy(scene.handle)  # the frame's render is still pending: it is settled here
            scene.handle = None
            assert np.array_equal(frame.download(), expect)
        else:
            lib.crh_frame_destroy(frame.handle)
            frame.handle = None
            assert scene.status() == 0


@pytest.mark.gpu
@pytest.mark.parametrize("seed", range(int(__import__("os").environ.get("CRH_FUZZ_API_SEEDS", "6"))))
def test_random_api_sequences_against_a_host_model(seed, oracle_lib):
    """Stateful sweep: random sequences of upload (fresh or into an existing Scene), instance updates, plain and recorded passes, passes
    over existing content (LoadOp::Load), dynamic stroke option updates and late downloads on two Scenes and two Frames of one Renderer.
    A host model replays every pass with the oracle; every download must equal it bit for bit."""
    import torch
    assert torch.cuda.is_available()
    from contrast_renderer_amd import Cap, DashInterval, DynamicStrokeOptions, Join
    from contrast_renderer_amd import renderer as R
    from oracle.binding import Oracle, render_pass
    rng = np.random.RandomState(4000 + seed)
    msaa = int(rng.choice([1, 4]))
    r = R.Renderer(R.Configuration(msaa, 2, 4, 2), device=0)
    sizes = [(int(rng.randint(60, 200)), int(rng.randint(60, 200))) for _ in range(2)]
    frames = [R.Frame(r, w, h) for w, h in sizes]
    model = [np.zeros((h, w, 4), dtype=np.uint8) for w, h in sizes]  # what each frame must hold
    cleared = [True, True]
    for f in frames:
        f.clear()
    gpu_scenes, host = [None, None], [None, None]  # host[i] = dict(batch, oracle, transforms, colors)

    def fresh_scene():
        while True:
            sc = scenes.scene_mixed(int(rng.randint(2, 25)), (160, 160), seed=int(rng.randint(0, 10000)))
            o = Oracle(sc["batch"])
            if o.status() == 0:
                return sc, o

    for step in range(40):
        op = rng.randint(0, 8)
        k = int(rng.randint(0, 2))
        if op == 0 or gpu_scenes[k] is None:  # upload: a fresh Scene, or new geometry into the existing one (existing_shape, renderer.rs:216-221)
            sc, o = fresh_scene()
            gpu_scenes[k] = R.Scene(r, sc["batch"], existing=gpu_scenes[k] if rng.uniform() < 0.6 else None)
            assert gpu_scenes[k].status() == 0
            host[k] = dict(batch=sc["batch"], oracle=o, transforms=sc["transforms"], colors=sc["colors"], instances_set=False)
        elif op == 1:  # new instance data
            n = host[k]["batch"].n_shapes
            host[k]["transforms"] = scenes.place(160, 160, rng.uniform(0, 160, n), rng.uniform(0, 160, n), rng.uniform(5, 70, n))
            host[k]["colors"] = np.concatenate([rng.uniform(0, 1, (n, 3)), rng.uniform(0.2, 1, (n, 1))], axis=1).astype(np.float32)
            gpu_scenes[k].set_instances(host[k]["transforms"], host[k]["colors"])
            host[k]["instances_set"] = True
        elif op in (2, 3, 4):  # a pass into frame j: cleared first or over what is there
            j = int(rng.randint(0, 2))
            w, h = sizes[j]
            if rng.uniform() < 0.6:
                frames[j].clear()
                cleared[j] = True
                model[j] = np.zeros_like(model[j])
            n = host[k]["batch"].n_shapes
            draws = [d for i in range(n) for d in ((i, i, int(Op.Stencil), 0, 0), (i, i, int(Op.Color), 0, 0))]
            if op == 4 and n >= 3:  # recorded: shape 0 clips the rest
                inner = [d for i in range(1, n) for d in ((i, i, int(Op.Stencil), 1, 0), (i, i, int(Op.Color), 1, 0))]
                draws = [(0, 0, int(Op.Stencil), 0, 0), (0, 0, int(Op.Clip), 1, 0)] + inner + [(0, 0, int(Op.UnClip), 0, 0)]
                gpu_scenes[k].render_draws(frames[j], host[k]["transforms"], host[k]["colors"], draws)
            else:
                if not host[k]["instances_set"] or rng.uniform() < 0.5:
                    gpu_scenes[k].render(frames[j], host[k]["transforms"], host[k]["colors"])
                    host[k]["instances_set"] = True
                else:
                    gpu_scenes[k].render(frames[j])
            model[j], _ = render_pass(host[k]["oracle"], w, h, msaa, 4, 2, 2, host[k]["transforms"], host[k]["colors"], draws, load=None if cleared[j] else model[j])
            cleared[j] = False
        elif op == 5:  # tessellate again (same geometry: the frames in flight must not notice), or clear a frame without drawing
            if rng.uniform() < 0.5:
                gpu_scenes[k].tessellate()
            else:
                j = int(rng.randint(0, 2))
                frames[j].clear()
                cleared[j] = True
                model[j] = np.zeros_like(model[j])
        elif op == 7:  # new dynamic stroke options for one group of one Shape (Shape::set_dynamic_stroke_options, renderer.rs:360-376): the passes in flight keep the old ones
            batch = host[k]["batch"]
            grouped = [s for s in range(batch.n_shapes) if batch.shape_dynamic_begin[s + 1] > batch.shape_dynamic_begin[s]]
            if not grouped:
                continue
            s = grouped[int(rng.randint(0, len(grouped)))]
            d0 = int(batch.shape_dynamic_begin[s])
            g = int(rng.randint(0, int(batch.shape_dynamic_begin[s + 1]) - d0))
            join, c0, c1 = Join(int(rng.randint(0, 3))), Cap(int(rng.randint(0, 7))), Cap(int(rng.randint(0, 7)))
            if batch.dynamic_stroke_options[d0 + g].dashed:  # (a dashed group stays dashed, a solid one solid)
                a, b = sorted(rng.uniform(0.3, 3.0, 2))
                new = DynamicStrokeOptions.Dashed(join, [DashInterval(float(a), float(b) + 0.2, c0, c1)], float(rng.uniform(-1, 1)))
            else:
                new = DynamicStrokeOptions.Solid(join, c0, c1)
            gpu_scenes[k].set_dynamic_stroke_options(s, g, new)
            batch.dynamic_stroke_options[d0 + g] = new.to_c()
            host[k]["oracle"] = Oracle(batch)
        else:  # a late download (a cleared frame is transparent)
            j = int(rng.randint(0, 2))
            assert np.array_equal(frames[j].download(), model[j]), f"seed {seed} step {step}: frame {j} differs"
    for j in range(2):
        assert np.array_equal(frames[j].download(), model[j]), f"seed {seed}: final frame {j} differs"


@pytest.mark.gpu
def test_malformed_batches_are_rejected_not_read_out_of_bounds(oracle_lib):
    """The C ABI cannot trust the index arrays of a crh_path_batch (the Rust types make these states unrepresentable): prefix arrays that
    do not start at 0, decrease or end beyond the element counts, segment types out of range, a float count that does not match the
    segment types, missing arrays — each is CRH_ERR_INVALID_ARGUMENT, and the valid batch still uploads afterwards."""
    import copy
    import ctypes as C
    import torch
    assert torch.cuda.is_available()
    from contrast_renderer_amd import _ffi
    from contrast_renderer_amd import renderer as R
    sc = scenes.scene_mixed(6, (128, 128), seed=3)
    batch = sc["batch"]
    r = R.Renderer(R.Configuration(1, 4, 4), device=0)
    lib = r.lib

    def upload(c_struct):
        handle = C.c_void_p()
        status = lib.crh_scene_upload(r.handle, C.byref(c_struct), None, C.byref(handle))
        if status == 0:
            lib.crh_scene_destroy(handle)
        return status

    assert upload(batch.c) == 0
    keep = []  # numpy arrays behind the patched pointers

    def variant(edit):
        c = _ffi.PathBatchC()
        C.memmove(C.byref(c), C.byref(batch.c), C.sizeof(c))
        edit(c)
        return c

    def patched(field, ctype, values):
        arr = np.ascontiguousarray(values)
        keep.append(arr)
        return lambda c: setattr(c, field, arr.ctypes.data_as(C.POINTER(ctype)))

    spb, psb = batch.shape_path_begin.copy(), batch.path_segment_begin.copy()
    cases = {
        "shape prefix does not start at 0": patched("shape_path_begin", C.c_uint32, spb + 1),
        "shape prefix decreases": patched("shape_path_begin", C.c_uint32, np.concatenate([spb[:2][::-1], spb[2:]]) if spb[1] > 0 else spb[::-1]),
        "shape prefix ends beyond the paths": patched("shape_path_begin", C.c_uint32, np.concatenate([spb[:-1], [spb[-1] + 5]]).astype(np.uint32)),
        "path prefix ends beyond the segments": patched("path_segment_begin", C.c_uint32, np.concatenate([psb[:-1], [psb[-1] + 1000]]).astype(np.uint32)),
        "path prefix decreases": patched("path_segment_begin", C.c_uint32, np.concatenate([[0, psb[-1]], psb[2:]]).astype(np.uint32)),
        "segment type out of range": patched("segment_types", C.c_uint8, np.where(np.arange(len(batch.segment_types)) == 3, 9, batch.segment_types).astype(np.uint8)),
        "float count too large": lambda c: setattr(c, "n_control_floats", c.n_control_floats + 7),
        "float count too small": lambda c: setattr(c, "n_control_floats", c.n_control_floats - 2),
        "segment count too large": lambda c: setattr(c, "n_segments", c.n_segments + 1),
        "no control data": lambda c: setattr(c, "control_data", C.POINTER(C.c_float)()),
        "no start points": lambda c: setattr(c, "path_start", C.POINTER(C.c_float)()),
        "dynamic options without a prefix": lambda c: setattr(c, "shape_dynamic_begin", C.POINTER(C.c_uint32)()),
        "stroke options index out of range": patched("path_stroke_options", C.c_int32, np.where(batch.path_stroke_options >= 0, 10 ** 6, batch.path_stroke_options).astype(np.int32)),
    }
    for name, edit in cases.items():
        assert upload(variant(edit)) == _ffi.ERR_INVALID_ARGUMENT, name
    assert upload(batch.c) == 0


@pytest.mark.gpu
@pytest.mark.parametrize("msaa", [1, 4])
def test_resubmitted_passes_with_moving_instances(msaa, oracle_lib):
    """An animation: the same recorded pass (clip nesting) and the same plain pass submitted frame after frame with new instance data,
    no host synchronisation in between, two frames alternating — the cached pass, the double-buffered instance sets and the upload
    stream. Every frame is downloaded only at the end and must equal the oracle's rendering of ITS instance data."""
    import torch
    assert torch.cuda.is_available()
    from contrast_renderer_amd import renderer as R
    from oracle.binding import Oracle, render_pass
    sc = scenes.scene_mixed(14, (160, 160), seed=21)
    o = Oracle(sc["batch"])
    assert o.status() == 0
    n = sc["batch"].n_shapes
    inner = [d for i in range(1, n) for d in ((i, i, int(Op.Stencil), 1, 0), (i, i, int(Op.Color), 1, 0))]
    recorded = np.array([(0, 0, int(Op.Stencil), 0, 0), (0, 0, int(Op.Clip), 1, 0)] + inner + [(0, 0, int(Op.UnClip), 0, 0)], dtype=np.uint32)
    plain = [d for i in range(n) for d in ((i, i, int(Op.Stencil), 0, 0), (i, i, int(Op.Color), 0, 0))]
    r = R.Renderer(R.Configuration(msaa, 2, 4, 0), device=0)
    scene = R.Scene(r, sc["batch"])
    rng = np.random.RandomState(5)
    for mode in ("recorded", "plain"):
        frames = [R.Frame(r, 160, 160) for _ in range(2)]
        shown = [None, None]
        for step in range(14):
            t = scenes.place(160, 160, rng.uniform(20, 140, n), rng.uniform(20, 140, n), rng.uniform(10, 60, n))
            c = np.concatenate([rng.uniform(0, 1, (n, 3)), rng.uniform(0.3, 1, (n, 1))], axis=1).astype(np.float32)
            f = frames[step & 1]
            f.clear()
            if mode == "recorded":
                scene.render_draws(f, t, c, recorded)
            else:
                scene.render(f, t, c)
            shown[step & 1] = (t, c)
            if step == 7:  # one download in the middle of the animation
                expect, _ = render_pass(o, 160, 160, msaa, 4, 2, 0, t, c, recorded.tolist() if mode == "recorded" else plain)
                assert np.array_equal(f.download(), expect)
        for k in range(2):
            t, c = shown[k]
            expect, _ = render_pass(o, 160, 160, msaa, 4, 2, 0, t, c, recorded.tolist() if mode == "recorded" else plain)
            assert np.array_equal(frames[k].download(), expect), f"{mode}: frame {k}"


# ---- Fill-only scenes, many Shapes, and the raster paths under every pin ---------------------------------------------------------------------

RASTER_VARIANTS = {0: "none", 1: "fill", 2: "edges", 3: "edges-long", 4: "rows", 5: "rows-long", 6: "tile", 7: "ops"}
BIN_ROUTES = {0: "none", 1: "triangles", 2: "flat", 3: "flat-batches", 4: "itemwise"}


def last_pass(frame):
    """crh_debug_frame_last_pass: what the frame's last pass ran (the formulation 1 edges / 2 triangles / 3 row spans, whether it was the
    Scene's measured choice, the general kernel, whether the Renderer pipelines its passes, the raster kernel variant, the binning route)."""
    import ctypes as C
    from contrast_renderer_amd import _ffi
    lib = frame.lib
    lib.crh_debug_frame_last_pass.restype = C.c_int
    lib.crh_debug_frame_last_pass.argtypes = [C.c_void_p, C.POINTER(C.c_uint32)]
    out = (C.c_uint32 * 4)()
    _ffi.check(lib.crh_debug_frame_last_pass(frame.handle, out))
    return dict(formulation=out[0] & 0xFF, measured=bool(out[0] & 256), general=out[1] & 1, pipelined=not out[1] & 256, raster=RASTER_VARIANTS[out[2]],
                bin=BIN_ROUTES[out[3] & 0xFF],
                direct=bool(out[3] & 256), ordered=bool(out[3] & 512), items=out[3] >> 16)


def _not_tile_multiple(v):
    return v + 1 if v % 16 == 0 else v


def fill_case(seed, many=False, n_frames=None):
    """Fill-only scenes (every fill segment type, no strokes): the paths of k_raster_fill, k_raster_rows and the measured choice between
    formulations. kind 0: plain instances drifting a little from frame to frame; 5: extreme placements; 1: perspective. `many`: 256 - 600
    small Shapes on a frame of at most 256^2 (a Scene choose_pass measures), plain instances, msaa 1 for even seeds and 4 for odd ones."""
    rng = np.random.RandomState((5000 if many else 3000) + seed)
    if many:
        width, height = _not_tile_multiple(int(rng.randint(120, 257))), _not_tile_multiple(int(rng.randint(120, 257)))
        n_shapes, msaa, kind = int(rng.randint(280, 601)), (1, 4)[seed % 2], 0  # (a few Shapes may go: without_failing_shapes)
        n_frames = n_frames or 24  # six per candidate of the trial (three at msaa 1) and the frames after the choice
    else:
        width, height = _not_tile_multiple(int(rng.randint(40, 300))), _not_tile_multiple(int(rng.randint(40, 300)))
        n_shapes, msaa, kind = int(rng.randint(3, 40)), (1, 4)[(seed // 3) % 2], (0, 5, 1)[seed % 3]
        n_frames = n_frames or 4
    winding_bits = int(rng.choice([1, 2, 4]))
    base = scenes.scene_mixed(n_shapes, (max(width, 96), max(height, 96)), seed=seed, fills_only=True)
    base["batch"] = without_failing_shapes(base["batch"])
    n = base["batch"].n_shapes
    frames = []
    if kind == 0:
        lo = 3.0 if many else 8.0
        cx, cy = rng.uniform(-10, width + 10, n), rng.uniform(-10, height + 10, n)
        scale = rng.uniform(lo, (12.0 if many else 0.5 * min(width, height)), n)
        vx, vy = rng.uniform(-1.5, 1.5, n), rng.uniform(-1.5, 1.5, n)
        for k in range(n_frames):
            frames.append(scenes.place(width, height, cx + k * vx, cy + k * vy, scale).astype(np.float32))
    for k in range(n_frames if kind != 0 else 0):
        if kind == 5:
            frames.append(scenes.place(width, height, rng.uniform(-3 * width, 4 * width, n), rng.uniform(-3 * height, 4 * height, n),
                                       np.exp(rng.uniform(math.log(0.05), math.log(40.0 * max(width, height)), n))).astype(np.float32))
        else:
            projection = utils.perspective_projection(math.pi * 0.5, width / height, 1.0, 100.0)
            frames.append(np.stack([utils.matrix_multiplication(projection, utils.matrix_multiplication(
                utils.translation_matrix(rng.uniform(-2, 2), rng.uniform(-2, 2), rng.uniform(0.8, 6.0)),
                utils.rotation_matrix(rng.uniform(-1.4, 1.4), (math.cos(i * 1.7), math.sin(i * 1.7), 0.0)))) for i in range(n)]).astype(np.float32))
    colors = np.concatenate([rng.uniform(0, 1, (n, 3)), rng.uniform(0.2, 1, (n, 1))], axis=1).astype(np.float32)
    colors[::2, 3] = 1.0  # (opaque covers: the late start of a tile's list)
    return dict(width=width, height=height, msaa=msaa, winding_bits=winding_bits, batch=base["batch"], frames=frames, colors=colors, kind=kind, many=many)


def without_failing_shapes(batch):
    """The fill-only batch without the Shapes the reference cannot tessellate (fill.rs:174,178 panic on them, and one fails the whole Scene)."""
    from contrast_renderer_amd import _ffi
    from oracle.binding import Oracle
    o = Oracle(batch)
    if o.status() == 0:
        return batch
    parts = [batch.slice_shapes(s, s + 1) for s in range(batch.n_shapes) if o.shape_status(s) == 0]
    spb, psb, starts, types, control = [0], [0], [], [], []
    for b in parts:
        spb += [spb[-1] + int(v) for v in b.shape_path_begin[1:]]
        psb += [psb[-1] + int(v) for v in b.path_segment_begin[1:]]
        starts.append(b.path_start), types.append(b.segment_types), control.append(b.control_data)
    return _ffi.PathBatch(spb, psb, np.concatenate(starts), -np.ones(spb[-1], np.int32), np.concatenate(types), np.concatenate(control))


def tess_marks(r, scene):
    """The timing marks of one more tessellation of `scene` (which tessellation path the Scene is on)."""
    r.enable_timing(True)
    scene.tessellate()
    r.synchronize()
    names = [name for name, _, _ in r.kernel_times()]
    r.enable_timing(False)
    return names


def check_fill_case(c, marks=False):
    """Every frame of the case drawn into one frame object (cleared in between) and compared with the oracle's image of ITS instances;
    plain placements (kind 0, not `many`) then upload the same paths again into the same Scene and draw the last frame once more.
    -> dict(taps=[the last_pass of every frame], upload=the last_pass after the upload or None, kernels=the tessellation's marks when `marks`)."""
    from contrast_renderer_amd import renderer as R
    from oracle.binding import Oracle
    o = Oracle(c["batch"])
    r = R.Renderer(R.Configuration(msaa_sample_count=c["msaa"], clip_nesting_counter_bits=2, winding_counter_bits=c["winding_bits"]), device=0)
    scene = R.Scene(r, c["batch"])
    assert scene.status() == o.status() == 0  # (without_failing_shapes)
    frame = R.Frame(r, c["width"], c["height"])
    taps = []
    for k, t in enumerate(c["frames"]):
        frame.clear()
        scene.render(frame, t, c["colors"])
        image = frame.download()
        expect = o.render(c["width"], c["height"], c["msaa"], c["winding_bits"], t, c["colors"])
        assert np.array_equal(image, expect), f"frame {k}: {(image != expect).any(axis=2).sum()} pixels differ ({last_pass(frame)})"
        taps.append(last_pass(frame))
    upload = None
    if c["kind"] == 0 and not c["many"]:  # the same structure uploaded again (existing_shape): the frame's list places and batch runs outlive it
        scene = R.Scene(r, c["batch"], existing=scene)
        frame.clear()
        scene.render(frame, c["frames"][-1], c["colors"])
        image = frame.download()
        assert np.array_equal(image, expect), f"after the upload: {(image != expect).any(axis=2).sum()} pixels differ ({last_pass(frame)})"
        upload = last_pass(frame)
    return dict(taps=taps, upload=upload, kernels=tess_marks(r, scene) if marks else None)


def _fill_seeds():
    return range(int(__import__("os").environ.get("CRH_FUZZ_FILL_SEEDS", "24")))


def _many_seeds():
    return range(int(__import__("os").environ.get("CRH_FUZZ_MANY_SEEDS", "4")))


def _no_path_pins(monkeypatch):
    """The tests that assert which path ran set their own pins: a pin of the whole suite's run (CRH_* but the seed counts) is cancelled
    for them — a run of the suite under a pin does not cover these tests under that pin."""
    import os
    for name in [v for v in os.environ if v.startswith("CRH_") and not v.startswith("CRH_FUZZ")]:
        monkeypatch.delenv(name)


@pytest.mark.gpu
@pytest.mark.parametrize("seed", _fill_seeds())
def test_random_fill_scene_matches_the_oracle_on_its_raster_path(seed, oracle_lib, monkeypatch):
    """Fill-only scenes, no pin: bit for bit on every frame, and on the path they are meant for — msaa 1 plain instances on k_raster_fill,
    msaa 4 on k_raster_edges, perspective on the general kernel; the lists in place and the measured batches of k_bin_flat from the later
    frames on."""
    import torch
    assert torch.cuda.is_available()
    _no_path_pins(monkeypatch)
    c = fill_case(seed)
    out = check_fill_case(c)
    taps = out["taps"] + ([out["upload"]] if out["upload"] else [])
    assert all(t["pipelined"] for t in taps), taps
    if c["kind"] == 1:
        assert all(t["general"] == 1 and t["raster"] == "ops" and t["formulation"] == 2 for t in taps), taps
        return
    plain = [t for t in taps if t["formulation"] == 1]
    if c["kind"] == 0:
        assert len(plain) == len(taps), taps  # (a Scene of fewer than 256 Shapes: always the edge formulation)
    for t in plain:
        assert t["general"] == 0 and t["raster"] == ("fill" if c["msaa"] == 1 else "edges"), taps
    if c["kind"] == 0:
        assert any(t["direct"] for t in taps) and any(t["ordered"] for t in taps), taps
        assert any(t["bin"] == "flat-batches" for t in taps) or all(t["bin"] == "itemwise" for t in taps), taps
        assert out["upload"]["direct"], out["upload"]  # (the lineage of the Scene's structure keeps the lists' places)


@pytest.mark.gpu
@pytest.mark.parametrize("seed", _many_seeds())
def test_many_shapes_through_the_measured_choice_of_formulation(seed, oracle_lib, monkeypatch):
    """256 - 600 small fill-only Shapes whose instances move every frame: choose_pass times six frames of each candidate (edges, triangles,
    and at msaa 1 row spans) and keeps the fastest. Every frame — each trial window and the frames after the choice — is the oracle's."""
    import torch
    assert torch.cuda.is_available()
    _no_path_pins(monkeypatch)
    c = fill_case(seed, many=True)
    assert c["batch"].n_shapes >= 256 and len(c["frames"]) >= 19
    taps = check_fill_case(c)["taps"]
    seen = {t["formulation"] for t in taps}
    assert seen >= ({1, 2, 3} if c["msaa"] == 1 else {1, 2}), taps
    assert any(t["measured"] for t in taps), [t["formulation"] for t in taps]
    for t in taps:
        assert t["general"] == 0
        if t["formulation"] == 3:
            assert t["raster"] in ("rows", "rows-long"), t
        elif t["formulation"] == 2:
            assert t["raster"] == "tile" and t["bin"] == "triangles", t
        else:
            assert t["raster"] == ("fill" if c["msaa"] == 1 else "edges"), t


# (pin, value, what it must show on the passes it reaches). Pins cached in a `static` (CRH_NO_SLAB_CULL, CRH_LOOPBACK_SERIAL, CRH_BIN_DUMP) are
# left out: set inside a running process they would not take effect.
PINS = [("CRH_TRIANGLE_PASS", "1"), ("CRH_EDGE_PASS", "1"), ("CRH_ROWS", "1"), ("CRH_FILL_KERNEL", "0"), ("CRH_LONG_LISTS", "0"), ("CRH_LONG_LISTS", "1"),
        ("CRH_NO_DIRECT_LISTS", "1"), ("CRH_NO_BIN_BATCHES", "1"), ("CRH_BIN_ITEMWISE", "1"), ("CRH_BIN_ITEMS", "1"), ("CRH_HEAVY_FIRST", "0"),
        ("CRH_TESS_TWO_PASS", "1"), ("CRH_NO_LINEAGE", "1"), ("CRH_NO_PIPELINE", "1")]
# both families, both sample counts: fill seeds 0 (plain, msaa 1), 3 (plain, msaa 4), 6 (plain, msaa 1), 1 (extreme, msaa 1), 2 (perspective,
# msaa 1), many-Shapes seed 0 (msaa 1), and two random_case seeds of the mixed family (strokes, recorded passes): 0 at msaa 1, 1 at msaa 4
PIN_CASES = [("fill", 0), ("fill", 3), ("fill", 6), ("fill", 1), ("fill", 2), ("many", 0), ("mixed", 0), ("mixed", 1)]


def test_the_pin_cases_cover_both_families_and_sample_counts():
    fams = {(fam, fill_case(s, many=fam == "many", n_frames=1)["msaa"] if fam != "mixed" else random_case(s)["msaa"]) for fam, s in PIN_CASES}
    assert {("fill", 1), ("fill", 4), ("many", 1), ("mixed", 1), ("mixed", 4)} <= fams, fams
    assert len(PIN_CASES) >= 8
    assert {fill_case(s)["kind"] for fam, s in PIN_CASES if fam == "fill"} == {0, 1, 5}


@pytest.mark.gpu
@pytest.mark.parametrize("case", PIN_CASES, ids=[f"{f}{s}" for f, s in PIN_CASES])
@pytest.mark.parametrize("pin", PINS, ids=[f"{n}={v}" for n, v in PINS])
def test_pinned_raster_paths_match_the_oracle(pin, case, oracle_lib, monkeypatch):
    """Every pin the library reads per pass, upload, launch or Renderer: the same frames, bit for bit, and the path the pin names is the
    one that ran (crh_debug_frame_last_pass; CRH_TESS_TWO_PASS: the tessellation's timing marks). CRH_NO_LINEAGE shows only after an upload
    of the same structure, which the plain fill cases make (fill0, fill3, fill6); on the other cases it is checked for pixels alone."""
    import torch
    assert torch.cuda.is_available()
    _no_path_pins(monkeypatch)
    name, value = pin
    monkeypatch.setenv(name, value)  # (before the Renderer is created: CRH_NO_PIPELINE is read there)
    family, seed = case
    marks = name == "CRH_TESS_TWO_PASS"
    if family == "mixed":
        out, msaa, fills = check_random_case(seed, marks=marks), random_case(seed)["msaa"], False
    else:
        c = fill_case(seed, many=family == "many", n_frames=6 if family == "many" else None)
        out, msaa, fills = check_fill_case(c, marks=marks), c["msaa"], True
    assert out is not None, "the pin cases are Scenes the reference tessellates"
    upload = out.get("upload")
    taps = out["taps"] + ([upload] if upload else [])
    if marks:
        assert "tess_emit" in out["kernels"] and "tess_fused" not in out["kernels"], out["kernels"]
    if family == "fill" and seed in (0, 3, 6):
        assert upload is not None
    plain = [t for t in taps if t["general"] == 0]
    edge = [t for t in plain if t["formulation"] != 2]
    if name == "CRH_TRIANGLE_PASS":
        assert all(t["formulation"] == 2 and t["raster"] == "tile" for t in plain), taps
    elif name == "CRH_EDGE_PASS":
        assert all(t["formulation"] in (1, 2) for t in plain) and all(t["raster"] in ("fill", "edges", "edges-long") for t in edge), taps
        assert edge or not plain, taps
    elif name == "CRH_ROWS":
        rows = fills and msaa == 1
        assert all(t["formulation"] in ((3, 2) if rows else (1, 2)) for t in plain), taps
        assert all(t["raster"] in (("rows", "rows-long") if rows else ("fill", "edges", "edges-long")) for t in edge), taps
        assert edge or not plain, taps
    elif name == "CRH_FILL_KERNEL":
        assert all(t["raster"] != "fill" for t in taps), taps
        if fills and msaa == 1:
            assert all(t["raster"] in ("edges", "edges-long") for t in edge), taps
    elif name == "CRH_LONG_LISTS" and value == "0":
        assert all(t["raster"] not in ("edges-long", "rows-long") for t in taps), taps
    elif name == "CRH_LONG_LISTS":
        if fills and msaa == 1:
            assert all(t["raster"] in ("fill", "edges-long", "rows-long") for t in edge), taps
    elif name == "CRH_NO_DIRECT_LISTS":
        assert not any(t["direct"] for t in taps), taps
    elif name == "CRH_NO_BIN_BATCHES":
        assert all(t["bin"] != "flat-batches" for t in taps), taps
    elif name == "CRH_BIN_ITEMWISE":
        assert all(t["bin"] == "itemwise" for t in edge), taps
    elif name == "CRH_BIN_ITEMS":
        assert all(t["items"] == 1 for t in edge if t["bin"] in ("flat", "itemwise")), taps
        assert any(t["bin"] in ("flat", "itemwise") for t in edge) or not edge, taps
    elif name == "CRH_HEAVY_FIRST":
        assert not any(t["ordered"] for t in taps), taps
    elif name == "CRH_NO_LINEAGE":
        if upload is not None:  # (the first pass after the upload: no list places, no batch runs of the paths before it)
            assert not upload["direct"] and upload["bin"] != "flat-batches", upload
    elif name == "CRH_NO_PIPELINE":
        assert not any(t["pipelined"] for t in taps), taps


def tile_aligned_case(seed):
    """Rectangles and triangles whose edges lie ON tile borders (multiples of 16 pixels) and on sample positions (+ 0.5), in pixel units
    on a power-of-two frame (the instance transform maps them to pixels exactly): the boundary cases of the binning kernels' tile-overlap tests."""
    from contrast_renderer_amd import Path, batch_from_shapes
    rng = np.random.RandomState(6000 + seed)
    width, height = 256, 128
    shapes = []
    for i in range(48):
        x0 = 16.0 * rng.randint(0, 15) + rng.choice([0.0, 0.0, 0.5, 8.0])
        y0 = 16.0 * rng.randint(0, 7) + rng.choice([0.0, 0.0, 0.5, 8.0])
        x1 = x0 + 16.0 * rng.randint(1, 5) + rng.choice([0.0, 0.0, -0.5, 8.0])
        y1 = y0 + 16.0 * rng.randint(1, 4) + rng.choice([0.0, 0.0, -0.5, 8.0])
        if i % 3 == 2:
            pts = [(x0, y0), (x1, y0), (x0 if i % 2 else x1, y1)]
            shapes.append(([], [Path.from_polygon(pts)]))
        else:
            shapes.append(([], [Path.from_rect(((x0 + x1) / 2, (y0 + y1) / 2), ((x1 - x0) / 2, (y1 - y0) / 2))]))
    batch = batch_from_shapes(shapes)
    t = np.tile(scenes.ortho_pixels(width, height), (len(shapes), 1)).astype(np.float32)
    colors = np.concatenate([rng.uniform(0, 1, (len(shapes), 3)), rng.uniform(0.3, 1, (len(shapes), 1))], axis=1).astype(np.float32)
    colors[::2, 3] = 1.0
    return width, height, batch, t, colors


BORDER_PATHS = [("default", None, 1), ("default", None, 4), ("triangles", ("CRH_TRIANGLE_PASS", "1"), 1), ("triangles", ("CRH_TRIANGLE_PASS", "1"), 4),
                ("rows", ("CRH_ROWS", "1"), 1), ("edges-kernel", ("CRH_FILL_KERNEL", "0"), 1), ("itemwise", ("CRH_BIN_ITEMWISE", "1"), 1),
                ("itemwise", ("CRH_BIN_ITEMWISE", "1"), 4)]  # (row spans: msaa 1 only; at msaa 4 the per-sample edge kernel is the default already)


def border_path_ran(path, msaa, t):
    """Did the pass `t` (last_pass) run the path `path` of BORDER_PATHS names?"""
    if path == "triangles":
        return t["formulation"] == 2 and t["raster"] == "tile" and t["bin"] == "triangles"
    if path == "rows":
        return t["formulation"] == 3 and t["raster"] in ("rows", "rows-long")
    if path == "edges-kernel":
        return t["formulation"] == 1 and t["raster"] in ("edges", "edges-long")
    if path == "itemwise":
        return t["formulation"] == 1 and t["bin"] == "itemwise"
    return t["formulation"] == 1 and t["raster"] == ("fill" if msaa == 1 else "edges")


@pytest.mark.gpu
@pytest.mark.parametrize("path,pin,msaa", BORDER_PATHS, ids=[f"{p}-msaa{m}" for p, _, m in BORDER_PATHS])
def test_edges_on_tile_borders_match_the_oracle(path, pin, msaa, oracle_lib, monkeypatch):
    """Edges exactly on the borders between tiles and on sample positions: every raster path bins them into the tiles they matter in,
    and the path the case names is the one that ran."""
    import torch
    assert torch.cuda.is_available()
    from contrast_renderer_amd import renderer as R
    from oracle.binding import Oracle
    _no_path_pins(monkeypatch)
    if pin:
        monkeypatch.setenv(*pin)
    for seed in range(3):
        width, height, batch, t, colors = tile_aligned_case(seed)
        o = Oracle(batch)
        assert o.status() == 0
        r = R.Renderer(R.Configuration(msaa_sample_count=msaa, winding_counter_bits=4), device=0)
        scene = R.Scene(r, batch)
        frame = R.Frame(r, width, height)
        expect = o.render(width, height, msaa, 4, t, colors)
        for k in range(3):  # the verified pass, then the lists in place and the measured batches
            frame.clear()
            scene.render(frame, t, colors)
            image = frame.download()
            assert np.array_equal(image, expect), f"seed {seed} pass {k}: {(image != expect).any(axis=2).sum()} pixels differ ({last_pass(frame)})"
            assert border_path_ran(path, msaa, last_pass(frame)), (seed, k, last_pass(frame))
