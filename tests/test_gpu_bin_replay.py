"""k_bin_flat's pass 3 as a replay of the hits pass 1 kept in LDS (csrc/bin_edges.hip, k_bin_flat<S, T, true>). Only the order of the
entries inside a tile's list may differ from the walk it replaces, and the raster kernels sort the lists: every frame here is compared byte for byte —
with the oracle's image, with CRH_BIN_REPLAY=0 (the walk again), with the item-wise kernel — through the verified first pass (pair stream) and the
steady passes behind it (lists in place), with the records capped (CRH_BIN_REPLAY_CAP: batches that fall back walk again, all or nothing per batch),
in a slab pass, at msaa 4, with the 64-thread workgroup and with instances that move until a verified pass recurs. The binning word
(crh_debug_frame_last_pass) says whether a pass replayed (bit 11) and, once the frame is downloaded, whether some batch of it fell back (bit 12).

The scene: 200 cubic paths of radius 8-128 on 512 x 512 — batches of one to seven items, rectangles up to 17 x 17 tiles, closed chains; larger than
256 x 256, so that the pool's limit and the queue are reachable."""
import contextlib
import ctypes as C
import os

import numpy as np
import pytest

from test_gpu_bin_lanes import bin_word, zoomed
from test_gpu_parity import gpu, make_renderer  # noqa: F401 (the module-scoped fixture and the helper of the parity tests)

pytestmark = pytest.mark.gpu

SIZE = 512
FRAMES = 5  # the verified pass, then four more: the lists in place from the second on
DIRECT, REPLAYED, FELL_BACK = 256, 2048, 4096  # bits of the binning word
FALLBACK_WORD = 77  # of the frame's flag words: batches whose pass 3 walked again
# The most hits one wavefront finds in a batch of the steady passes of this scene at msaa 1 (128-thread workgroups, batches cut by cost): read from the
# workgroup records of a -DCRH_ABLATE build (tools/bin_phases.py's dump). A cap one below it makes exactly the batches with such a wavefront fall back.
LARGEST_WAVE_HITS = 565
# ... and the distribution of that figure over the 33 batches of a steady pass: 169 in the lightest batch, 369 in the median one (a verified first pass takes
# one item per workgroup: 32 to 241). No wavefront of this scene stays within 8 hits, so CRH_BIN_REPLAY_CAP=8 makes every batch walk again here; a cap at the
# median is the one that mixes batches that replay with batches that do not.
MEDIAN_WAVE_HITS = 369
PINS = ("CRH_BIN_REPLAY", "CRH_BIN_REPLAY_CAP", "CRH_BIN_ITEMWISE", "CRH_BIN_FLAT_THREADS", "CRH_NO_BIN_BATCHES", "CRH_BIN_ITEMS", "CRH_BIN_BATCH_ITEMS", "CRH_BIN_BATCH_TICKS",
        "CRH_NO_DIRECT_LISTS", "CRH_RASTER_DEBUG")


@contextlib.contextmanager
def pinned(**env):
    """The edge pass with k_bin_flat and nothing else pinned but `env` (every switch is read per launch)."""
    before = {k: os.environ.get(k) for k in PINS + ("CRH_EDGE_PASS", "CRH_BIN_FLAT")}
    for k in PINS:
        os.environ.pop(k, None)
    os.environ["CRH_EDGE_PASS"] = "1"
    os.environ["CRH_BIN_FLAT"] = "1"
    os.environ.update({k: str(v) for k, v in env.items()})
    try:
        yield
    finally:
        for k, v in before.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def cubic_scene():
    from contrast_renderer_amd import scenes
    return scenes.scene_cubic_fill(200, (SIZE, SIZE), r_lo=8.0, r_hi=128.0)


def flag_words(frame):
    """The 128 flag and counter words of the binning set of the frame's last pass (waits for the renderer)."""
    from contrast_renderer_amd import _ffi
    lib = frame.lib
    lib.crh_debug_frame_words.restype = C.c_int
    lib.crh_debug_frame_words.argtypes = [C.c_void_p, C.POINTER(C.c_uint32)]
    out = (C.c_uint32 * 128)()
    _ffi.check(lib.crh_debug_frame_words(frame.handle, out))
    return [int(w) for w in out]


def fallbacks(frame):
    """Batches of the frame's last pass that walked again."""
    return flag_words(frame)[FALLBACK_WORD]


def draw(gpu, msaa=1, frames=FRAMES, rows=None, views=None, **env):  # noqa: F811
    """`frames` passes of the scene into one frame -> [(image, binning word, batches that fell back)] per pass; views: the transforms of every pass."""
    sc = cubic_scene()
    with pinned(**env):
        r = make_renderer(gpu, msaa, 4)
        scene = gpu.Scene(r, sc["batch"])
        assert scene.status() == 0
        frame = gpu.Frame(r, SIZE, SIZE)
        if rows is not None:
            frame.set_tile_rows(*rows)
        out = []
        for k in range(frames):
            frame.clear()
            scene.render(frame, sc["transforms"] if views is None else views[k], sc["colors"])
            image = frame.download()
            out.append((image, bin_word(frame)[0], fallbacks(frame)))
        assert scene.status() == 0
    return out


@pytest.fixture(scope="module")
def expect(oracle_lib):
    sc = cubic_scene()
    return oracle_lib.Oracle(sc["batch"], 4).render(SIZE, SIZE, 1, 4, sc["transforms"], sc["colors"])


@pytest.fixture(scope="module")
def default_run(gpu):  # noqa: F811
    return draw(gpu)


def assert_frames(run, expect, what):
    for k, (image, _, _) in enumerate(run):
        assert np.array_equal(image, expect), f"{what}, pass {k}: {(image != expect).any(axis=2).sum()} pixels differ"


# ---------------------------------------------------------------------------------------------- replay against the other binning paths
def test_the_default_replays_every_batch_and_draws_the_oracles_frame(default_run, expect):
    assert_frames(default_run, expect, "replay")
    for k, (_, word, fell_back) in enumerate(default_run):
        assert word & REPLAYED, (k, hex(word))
        assert not (word & FELL_BACK) and fell_back == 0, (k, hex(word), fell_back)
    assert all(word & DIRECT for _, word, _ in default_run[2:]), "the steady passes store into the lists in place"


def test_a_first_pass_into_a_fresh_frame_replays_through_the_pair_stream(default_run, expect):
    image, word, fell_back = default_run[0]
    assert not (word & DIRECT) and (word & REPLAYED) and fell_back == 0, hex(word)
    assert np.array_equal(image, expect)


@pytest.mark.parametrize("env", [dict(CRH_BIN_REPLAY=0), dict(CRH_BIN_ITEMWISE=1)], ids=["walk-again", "itemwise"])
def test_replay_equals_the_other_binning_paths(gpu, default_run, expect, env):  # noqa: F811
    other = draw(gpu, **env)
    assert_frames(other, expect, str(env))
    for k, ((image, _, _), (mine, _, _)) in enumerate(zip(other, default_run)):
        assert np.array_equal(image, mine), k
    assert all(not (word & (REPLAYED | FELL_BACK)) and fell_back == 0 for _, word, fell_back in other), [hex(w) for _, w, _ in other]


# ---------------------------------------------------------------------------------------------- capacity caps
def test_cap_zero_makes_every_batch_walk_again(gpu, expect):  # noqa: F811
    run = draw(gpu, CRH_BIN_REPLAY_CAP=0)
    assert_frames(run, expect, "cap 0")
    assert all((word & REPLAYED) and (word & FELL_BACK) and fell_back > 0 for _, word, fell_back in run), [(hex(w), n) for _, w, n in run]


@pytest.mark.parametrize("cap", [8, MEDIAN_WAVE_HITS])
def test_a_small_cap_draws_the_same_frames_and_reports_its_fallbacks(gpu, expect, cap):  # noqa: F811
    every = draw(gpu, CRH_BIN_REPLAY_CAP=0)  # (every batch with a hit falls back: their number)
    run = draw(gpu, CRH_BIN_REPLAY_CAP=cap)
    assert_frames(run, expect, f"cap {cap}")
    for k, ((_, word, fell_back), (_, _, batches)) in enumerate(zip(run, every)):
        if k == 0 and cap == MEDIAN_WAVE_HITS:
            continue  # (the verified pass takes one item per workgroup: few or none of those reach the median of the steady batches)
        assert (word & REPLAYED) and (word & FELL_BACK), (k, hex(word))
        assert 0 < fell_back <= batches, (k, fell_back, batches)
        if cap == MEDIAN_WAVE_HITS:  # some batches replay and some do not
            assert fell_back < batches, (k, fell_back, batches)
    if cap == MEDIAN_WAVE_HITS:
        assert all(fell_back == 16 and batches == 33 for (_, _, fell_back), (_, _, batches) in zip(run[2:], every[2:])), [(a[2], b[2]) for a, b in zip(run, every)]


def test_a_cap_just_below_the_largest_wavefront_makes_that_batch_walk_again(gpu, expect):  # noqa: F811
    at = draw(gpu, CRH_BIN_REPLAY_CAP=LARGEST_WAVE_HITS)
    below = draw(gpu, CRH_BIN_REPLAY_CAP=LARGEST_WAVE_HITS - 1)
    assert_frames(at, expect, "cap at the largest wavefront")
    assert_frames(below, expect, "cap below the largest wavefront")
    assert all(fell_back == 0 and not (word & FELL_BACK) for _, word, fell_back in at[2:]), [(hex(w), n) for _, w, n in at]
    assert all(fell_back >= 1 and (word & FELL_BACK) for _, word, fell_back in below[2:]), [(hex(w), n) for _, w, n in below]


# ---------------------------------------------------------------------------------------------- single cases
def test_the_64_thread_workgroup(gpu, default_run, expect):  # noqa: F811
    run = draw(gpu, CRH_BIN_FLAT_THREADS=64)  # (whichever pass 3 that build has)
    assert_frames(run, expect, "64 threads")
    assert all(fell_back == 0 for _, _, fell_back in run)


def test_a_slab_pass_over_the_middle_third(gpu, expect):  # noqa: F811
    rows = (160, 352)  # whole 16-pixel tile rows
    masked = np.zeros_like(expect)
    masked[rows[0]:rows[1]] = expect[rows[0]:rows[1]]
    run, walk = draw(gpu, rows=rows), draw(gpu, rows=rows, CRH_BIN_REPLAY=0)
    assert_frames(run, masked, "slab, replay")
    assert_frames(walk, masked, "slab, walk again")
    assert all((word & REPLAYED) and fell_back == 0 for _, word, fell_back in run)


def test_msaa_4(gpu, oracle_lib):  # noqa: F811
    sc = cubic_scene()
    expect4 = oracle_lib.Oracle(sc["batch"], 4).render(SIZE, SIZE, 4, 4, sc["transforms"], sc["colors"])
    run = draw(gpu, msaa=4)
    assert_frames(run, expect4, "msaa 4")
    assert all(word & REPLAYED for _, word, _ in run)
    assert_frames(draw(gpu, msaa=4, frames=3, CRH_BIN_REPLAY_CAP=8), expect4, "msaa 4, cap 8")


# ---------------------------------------------------------------------------------------------- moving instances
def test_moving_instances_through_a_verified_pass_that_recurs(gpu, oracle_lib):  # noqa: F811
    """A zoom to a quarter between two passes brings all 200 paths into the 64 tiles at the centre, whose lists outgrow the places they were given (the pass
    is drawn again the verified way, through the pair stream); small steps keep their places: six frames, each the CRH_BIN_REPLAY=0 frame of the same
    view, the last one the oracle's."""
    sc = cubic_scene()
    views = [zoomed(sc["transforms"], z) for z in (1.0, 1.0, 1.01, 0.25, 0.26, 1.0)]
    run, walk = draw(gpu, frames=6, views=views), draw(gpu, frames=6, views=views, CRH_BIN_REPLAY=0)
    for k, ((image, word, _), (other, _, _)) in enumerate(zip(run, walk)):
        assert word & REPLAYED, (k, hex(word))
        assert np.array_equal(image, other), f"view {k}: {(image != other).any(axis=2).sum()} pixels differ"
    assert any(not (word & DIRECT) for _, word, _ in run[2:]), "a verified pass recurs"
    last = oracle_lib.Oracle(sc["batch"], 4).render(SIZE, SIZE, 1, 4, views[-1], sc["colors"])
    assert np.array_equal(run[-1][0], last)
