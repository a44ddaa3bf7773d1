"""Two binning lanes (CRH_BIN_LANES=2, read when the renderer is created): consecutive passes of a renderer bin on two streams
in turn, and two consecutive STEADY passes are not ordered against each other. Whatever the lanes do, every observable frame is the oracle's
image, bit for bit, and equals what the library draws with one lane (CRH_BIN_LANES=1, and the default: two lanes measured slower). The route
word (crh_debug_frame_last_pass, bit 10 of the binning word) says which passes ran unordered: only steady ones behind steady ones."""
import os

import numpy as np
import pytest

from test_gpu_parity import gpu, make_renderer  # noqa: F401 (the module-scoped fixture and the helper of the parity tests)

pytestmark = pytest.mark.gpu

STEPS = 40
UNORDERED = 1024  # last_bin: this pass' binning was not ordered behind the binning of the pass before it


def bin_word(frame):
    import ctypes as C
    from contrast_renderer_amd import _ffi
    lib = frame.lib
    lib.crh_debug_frame_last_pass.restype = C.c_int
    lib.crh_debug_frame_last_pass.argtypes = [C.c_void_p, C.POINTER(C.c_uint32)]
    out = (C.c_uint32 * 4)()
    _ffi.check(lib.crh_debug_frame_last_pass(frame.handle, out))
    return int(out[3]), int(out[0]) & 0xFF


def renderer_with_lanes(gpu, lanes, msaa=1, winding_bits=4):  # noqa: F811
    """CRH_BIN_LANES is read when the renderer is created: set around the creation only."""
    before = os.environ.get("CRH_BIN_LANES")
    if lanes is None:
        os.environ.pop("CRH_BIN_LANES", None)
    else:
        os.environ["CRH_BIN_LANES"] = str(lanes)
    try:
        return make_renderer(gpu, msaa, winding_bits)
    finally:
        if before is None:
            os.environ.pop("CRH_BIN_LANES", None)
        else:
            os.environ["CRH_BIN_LANES"] = before


def cubic_scene():
    from contrast_renderer_amd import scenes
    return scenes.scene_cubic_fill(600, (512, 512), r_lo=6.0, r_hi=50.0)


def zoomed(transforms, z):
    t = transforms.copy()
    t[:, [0, 1, 4, 5, 12, 13]] *= np.float32(z)
    return t


@pytest.fixture(scope="module")
def cubic_expect(oracle_lib):
    sc = cubic_scene()
    return oracle_lib.Oracle(sc["batch"], 4).render(512, 512, 1, 4, sc["transforms"], sc["colors"])


def steady_loop(gpu, lanes):  # noqa: F811
    """Test 1's loop: forty un-synchronised steps of tessellate / clear / render into ONE frame -> (image, status, [(binning word, formulation) per step])."""
    sc = cubic_scene()
    r = renderer_with_lanes(gpu, lanes)
    scene = gpu.Scene(r, sc["batch"])
    frame = gpu.Frame(r, 512, 512)
    scene.set_instances(sc["transforms"], sc["colors"])
    words = []
    for _ in range(STEPS):
        scene.tessellate()
        frame.clear()
        scene.render(frame)
        words.append(bin_word(frame))
    image = frame.download()
    return image, scene.status(), words


@pytest.fixture(scope="module", params=[None, "CRH_EDGE_PASS"], ids=["measured-choice", "edge-pass"])
def loops(request, gpu):  # noqa: F811
    """The loop with two lanes, with one and with the default, once with the Scene's measured choice of formulation and once pinned to the edge
    pass (the formulation of the steady path: what the measurement picks for 600 Shapes is the machine's business)."""
    pin = request.param
    before = os.environ.get(pin) if pin else None
    if pin:
        os.environ[pin] = "1"
    try:
        return pin, steady_loop(gpu, 2), steady_loop(gpu, 1), steady_loop(gpu, None)
    finally:
        if pin:
            if before is None:
                os.environ.pop(pin, None)
            else:
                os.environ[pin] = before


def test_steady_loop_into_one_target(loops, cubic_expect):
    pin, two, one, default = loops
    for name, (image, status, _) in (("two lanes", two), ("one lane", one), ("the default", default)):
        assert status == 0, name
        assert np.array_equal(image, cubic_expect), f"{name}: {(image != cubic_expect).any(axis=2).sum()} pixels differ"
    assert np.array_equal(two[0], one[0]) and np.array_equal(default[0], one[0])


def test_route_word_of_the_steady_loop(loops):
    pin, two, one, default = loops
    assert all(not (word & UNORDERED) for word, _ in one[2]), "one lane: every pass is ordered"
    assert all(not (word & UNORDERED) for word, _ in default[2]), "the default is one lane"
    assert not (two[2][0][0] & UNORDERED) and not (two[2][1][0] & UNORDERED), "the first passes are verified ones"
    late = two[2][STEPS - 8:]
    for word, formulation in late:
        steady = formulation in (1, 3) and bool(word & 256)  # the edge pass with its lists in place
        assert bool(word & UNORDERED) == steady, (pin, hex(word), formulation)
    if pin:
        assert all(word & UNORDERED for word, _ in late), [hex(w) for w, _ in late]


def test_two_targets_in_turn_with_moving_instances(gpu, oracle_lib):  # noqa: F811
    """The same loop into TWO frames drawn in turn, new instance transforms every step (a zoom of 1 %): the places of the lists are written
    again behind the binning kernels (or the pass is a verified one), so every one of these passes is an ordered one, on alternating lanes, with
    the instance copies on the lane of the pass that reads them. Each frame's final download is the oracle's render of the last view drawn into it."""
    sc = cubic_scene()
    oracle = oracle_lib.Oracle(sc["batch"], 4)
    r = renderer_with_lanes(gpu, 2)
    scene = gpu.Scene(r, sc["batch"])
    frames = [gpu.Frame(r, 512, 512) for _ in range(2)]
    views = [zoomed(sc["transforms"], 1.01 ** (k + 1)) for k in range(STEPS)]
    drawn = [None, None]
    for k, view in enumerate(views):
        f = frames[k % 2]
        scene.tessellate()
        scene.set_instances(view, sc["colors"])
        f.clear()
        scene.render(f)
        assert not (bin_word(f)[0] & UNORDERED), k
        drawn[k % 2] = view
    assert scene.status() == 0
    for which in range(2):
        got = frames[which].download()
        expect = oracle.render(512, 512, 1, 4, drawn[which], sc["colors"])
        assert np.array_equal(got, expect), f"target {which}: {(got != expect).any(axis=2).sum()} pixels differ"


def test_route_word_stays_clear_where_a_pass_must_be_ordered(gpu, oracle_lib, cubic_expect, monkeypatch):  # noqa: F811
    """Behind set_instances, a verified pass (drawn over existing content), a recorded pass and a frame restricted to a slab of tile rows
    the binning is ordered behind the pass before it — and the passes around them still draw the oracle's frame."""
    monkeypatch.setenv("CRH_EDGE_PASS", "1")
    sc = cubic_scene()
    oracle = oracle_lib.Oracle(sc["batch"], 4)
    r = renderer_with_lanes(gpu, 2)
    scene = gpu.Scene(r, sc["batch"])
    frame = gpu.Frame(r, 512, 512)
    scene.set_instances(sc["transforms"], sc["colors"])

    def step(clear=True):
        scene.tessellate()
        if clear:
            frame.clear()
        scene.render(frame)
        return bin_word(frame)[0]

    words = [step() for _ in range(10)]
    assert words[-1] & UNORDERED and words[-2] & UNORDERED, [hex(w) for w in words]
    # new instances: the places are rewritten behind this pass' binning kernel
    view = zoomed(sc["transforms"], 1.03)
    scene.set_instances(view, sc["colors"])
    assert not (step() & UNORDERED)
    assert not (step() & UNORDERED), "the pass behind one that rewrote the places waits for it"
    assert step() & UNORDERED
    got = frame.download()
    expect = oracle.render(512, 512, 1, 4, view, sc["colors"])
    assert np.array_equal(got, expect), f"after set_instances: {(got != expect).any(axis=2).sum()} pixels differ"
    scene.set_instances(sc["transforms"], sc["colors"])
    for _ in range(4):
        step()
    assert step() & UNORDERED
    # a verified pass: drawn over existing content, its pair count is read back before the raster kernel runs
    frame.clear()
    scene.render(frame)
    assert not (step(clear=False) & UNORDERED)
    assert not (step() & UNORDERED), "the pass behind a verified one waits for it"
    for _ in range(3):
        step()
    assert step() & UNORDERED
    assert np.array_equal(frame.download(), cubic_expect)
    # a recorded pass (crh_scene_render_draws): Stencil + Color of every Shape, as the plain pass draws them
    from contrast_renderer_amd.renderer import RenderOperation
    draws = [(i, i, op, 0, 0) for i in range(scene.n_shapes) for op in (RenderOperation.Stencil, RenderOperation.Color)]
    step()
    scene.tessellate()
    frame.clear()
    scene.render_draws(frame, sc["transforms"], sc["colors"], draws)
    assert not (bin_word(frame)[0] & UNORDERED)
    assert np.array_equal(frame.download(), cubic_expect)
    # a frame with a slab of tile rows
    slab = gpu.Frame(r, 512, 512)
    slab.set_tile_rows(128, 384)
    for _ in range(6):
        scene.tessellate()
        slab.clear()
        scene.render(slab)
        assert not (bin_word(slab)[0] & UNORDERED)
    got = slab.download()
    assert np.array_equal(got[128:384], cubic_expect[128:384]), f"slab: {(got[128:384] != cubic_expect[128:384]).any(axis=2).sum()} pixels differ"
    assert scene.status() == 0


def test_mixed_sequence_of_two_scenes_and_two_frames(gpu, oracle_lib):  # noqa: F811
    """Steady steps, set_instances, a re-upload into an existing Scene, frame.synchronize() and a download in the middle, interleaved over
    two Scenes (the second at its own msaa) and two frames: after every download the frame is the oracle's."""
    from contrast_renderer_amd import scenes
    a = scenes.scene_cubic_fill(400, (512, 512), r_lo=6.0, r_hi=50.0)
    a2 = scenes.scene_cubic_fill(400, (512, 512), r_lo=6.0, r_hi=50.0, first_path=400)
    b = scenes.scene_mixed(48, (512, 512), seed=21)
    ra = renderer_with_lanes(gpu, 2)
    rb = renderer_with_lanes(gpu, 2, b["msaa"], b["winding_bits"])
    oracle_a, oracle_a2, oracle_b = oracle_lib.Oracle(a["batch"], 4), oracle_lib.Oracle(a2["batch"], 4), oracle_lib.Oracle(b["batch"])
    scene_a, scene_b = gpu.Scene(ra, a["batch"]), gpu.Scene(rb, b["batch"])
    frame_a, frame_b = gpu.Frame(ra, 512, 512), gpu.Frame(rb, 512, 512)
    view_a, view_b = a["transforms"], b["transforms"]
    scene_a.set_instances(view_a, a["colors"])
    scene_b.set_instances(view_b, b["colors"])

    def steps(n):
        for _ in range(n):
            scene_a.tessellate()
            frame_a.clear()
            scene_a.render(frame_a)
            scene_b.tessellate()
            frame_b.clear()
            scene_b.render(frame_b)

    def check(what, oa=oracle_a, colors_a=a["colors"]):
        got = frame_a.download()
        expect = oa.render(512, 512, 1, 4, view_a, colors_a)
        assert np.array_equal(got, expect), f"{what}, first Scene: {(got != expect).any(axis=2).sum()} pixels differ"
        got = frame_b.download()
        expect = oracle_b.render(512, 512, b["msaa"], b["winding_bits"], view_b, b["colors"])
        assert np.array_equal(got, expect), f"{what}, second Scene: {(got != expect).any(axis=2).sum()} pixels differ"

    steps(16)
    check("steady steps")
    steps(3)
    view_a = zoomed(a["transforms"], 1.05)
    scene_a.set_instances(view_a, a["colors"])
    steps(2)
    view_b = zoomed(b["transforms"], 0.97)
    scene_b.set_instances(view_b, b["colors"])
    steps(5)
    frame_a.synchronize()
    steps(4)
    check("set_instances and synchronize")
    steps(2)
    scene_a = gpu.Scene(ra, a2["batch"], existing=scene_a)  # new paths into the Scene the frames in flight were drawn from
    view_a = a2["transforms"]
    scene_a.set_instances(view_a, a2["colors"])
    steps(18)
    frame_b.synchronize()
    steps(3)
    check("a re-upload", oracle_a2, a2["colors"])
    assert scene_a.status() == 0 and scene_b.status() == 0
