"""What the tests of the multi-GPU exchange share beside the host model (tests/exchange_model.py): the comparison of a group's traffic figures
with the model's, Scenes of pixel-aligned rectangles, and the deep equality of generated op lists."""
import numpy as np

from contrast_renderer_amd import Path, batch_from_shapes
from contrast_renderer_amd import renderer as R


def assert_traffic(comms, expected, where=""):
    for k, (c, e) in enumerate(zip(comms, expected)):
        assert c.last_peer_bytes() == e["peer_bytes"], f"{where}: rank {k}'s peer bytes {c.last_peer_bytes()}, the model's {e['peer_bytes']}"
        assert c.last_traffic() == (e["sent"], e["dense"]), f"{where}: rank {k}'s traffic {c.last_traffic()}, the model's {(e['sent'], e['dense'])}"


def pixel_transform(width, height):
    """Path coordinates = pixel coordinates, y down: path (x, y) is the corner of pixel (column x, row y)."""
    t = np.zeros(16, dtype=np.float32)
    t[0], t[5], t[10], t[15], t[12], t[13] = 2.0 / width, -2.0 / height, 1.0, 1.0, -1.0, 1.0
    return t


def rect_scene(r, width, height, rects):
    """One Shape per rectangle (x0, y0, x1, y1) -> (Scene, transforms [n, 16])."""
    scene = R.Scene(r, batch_from_shapes([([], [Path.from_rect(((x0 + x1) / 2.0, (y0 + y1) / 2.0), ((x1 - x0) / 2.0, (y1 - y0) / 2.0))]) for x0, y0, x1, y1 in rects]))
    assert scene.status() == 0
    return scene, np.tile(pixel_transform(width, height), (len(rects), 1))


def same(a, b):
    if isinstance(a, dict):
        return a.keys() == b.keys() and all(same(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple)):
        return len(a) == len(b) and all(same(x, y) for x, y in zip(a, b))
    if isinstance(a, np.ndarray):
        return isinstance(b, np.ndarray) and a.dtype == b.dtype and np.array_equal(a, b)
    return a == b
