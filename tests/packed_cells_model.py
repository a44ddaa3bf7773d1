"""Stacks of axis-aligned rectangles whose image is integer arithmetic (tests/test_gpu_packed_cells.py). Plain numpy, no product code.

A stack lives in a 64 x 64 frame. Rectangle k of a stack spans x in [left_k, RIGHT] and every row of the frame (its top, bottom and right
edges lie outside the frame), so only its LEFT edge crosses tiles of the frame: one list entry per rectangle in the tiles of the column
that holds the left edges, one backdrop unit per rectangle in the tiles to the right of it. left_k = BASE + shift + j_k * 2^-12 with
integers j_k that are no multiple of 256, so no edge lies on a sixteenth of a pixel — the sample positions of msaa 1 (x + 8/16) and of msaa 4
(x + 2, 6, 10, 14 sixteenths) are all sixteenths. Every coordinate is a multiple of 2^-12 below 128 in magnitude (19 bits), and so is
every intermediate of the instance transform of `transform` (a scale of exactly one pixel, a translation by a multiple of 2^-12 pixel):
binary32 places every vertex exactly, and the winding number of a sample is a COUNT — the clockwise rectangles whose left edge lies left of
it minus the reversed ones. No sample is near an edge in any sense that needs a tolerance: `counts` asserts that none is ON one."""
import numpy as np

SIZE = 64            # the frame, pixels (4 x 4 tiles of 16 x 16)
STEP = 2.0 ** -12    # the stagger, pixels
BASE = 17.0          # left edges start here: tile column 1 (x in [16, 32)) holds BASE + (0, 8.1]
RIGHT, TOP, BOTTOM = 100.0, -8.0, 72.0  # pixels (y down): outside the frame, also for a stack shifted by -16 .. +64 pixels
SAMPLE_X = {1: np.array([8.0]) / 16.0, 4: np.array([6.0, 14.0, 2.0, 10.0]) / 16.0}  # x offsets of the samples in sample-index order


def staggers(k, stride=1):
    """The first k admissible j, ascending: j = stride * i + 1 that are no multiple of 256, without the first one of every second band
    between two msaa-1 sample columns — so that the parity of the number of edges left of a column changes from column to column (at
    winding_counter_bits 1 a stack of equal signs is then neither drawn everywhere nor nowhere)."""
    out, i, last_band = [], 0, -1
    while len(out) < k:
        j = stride * i + 1
        i += 1
        if j % 256 == 0:
            continue
        band = int(np.floor(j * STEP + 0.5))
        if band != last_band:
            last_band = band
            if band % 2 == 0:
                continue
        out.append(j)
    return np.array(out, dtype=np.int64)


def stride_for(k):
    """A power of two that spreads k rectangles over about 8 pixels (so that the running count changes between sample columns)."""
    stride = 1
    while 2 * stride * k * STEP <= 8.0:
        stride *= 2
    return stride


def mixed_signs(j, bits):
    """Signs for the ascending staggers j such that the running count (the winding number just right of each left edge) swings deeply both
    ways inside every band between two msaa-1 sample columns and lands, AT those columns, on the targets 2^bits, 0, -1, -2^bits, -2 * 2^bits - 1,
    -2 * 2^bits, 3, 2 * 2^bits, ... in turn (a target further away than a band can move is approached over several bands). -> (keep, signs):
    keep drops at most one rectangle per band (the parity of a band's sum is the parity of its size)."""
    m = 1 << bits
    targets = [m, 0, -1, -m, -2 * m - 1, -2 * m, 3, 2 * m, 1, -3 * m]
    band = np.floor(j * STEP + 0.5).astype(np.int64)  # band c: the edges between sample columns c - 1 and c
    keep, signs, total, t = [], [], 0, 0
    for c in range(int(band.max()) + 1):
        idx = np.flatnonzero(band == c)
        if len(idx) == 0:
            continue
        if c == 0 or c == band.max():  # the first band rises as far as it can, the last (partial) one too
            keep.append(idx), signs.append(np.ones(len(idx), dtype=np.int64))
            total += len(idx)
            continue
        want = targets[t % len(targets)] - total
        if (want - len(idx)) % 2:
            idx = idx[:-1]
        n = len(idx)
        s = max(-n, min(n, want))
        if (s - n) % 2:
            s -= 1 if s > 0 else -1
        if s == want:
            t += 1
        plus = (n + s) // 2
        keep.append(idx), signs.append(np.concatenate([np.ones(plus, dtype=np.int64), -np.ones(n - plus, dtype=np.int64)]))
        total += s
    return np.concatenate(keep), np.concatenate(signs)


class Stack:
    """One Shape: rectangles with left edges BASE + j * STEP (+ the instance's shift), signs +1 (clockwise) / -1 (reversed)."""

    def __init__(self, j, signs, color=(1.0, 1.0, 1.0, 1.0), shift=0.0):
        self.j, self.signs, self.color, self.shift = np.asarray(j, dtype=np.int64), np.asarray(signs, dtype=np.int64), tuple(color), float(shift)
        assert len(self.j) == len(self.signs) and (self.j % 256 != 0).all() and (self.j > 0).all() and self.j.max() * STEP < 14.9
        assert self.shift * 4096.0 == round(self.shift * 4096.0) and -16.0 <= self.shift <= 64.0

    def lefts(self, shift=None):
        return BASE + (self.shift if shift is None else shift) + self.j * STEP

    def polygons(self):
        """Vertices in y-up path coordinates (pixels relative to the frame's centre), clockwise for +1: up the left edge first."""
        lo, hi, r = SIZE / 2 - BOTTOM, SIZE / 2 - TOP, RIGHT - SIZE / 2
        out = []
        for x, s in zip(BASE + self.j * STEP - SIZE / 2, self.signs):
            cw = [(x, lo), (x, hi), (r, hi), (r, lo)]
            out.append(cw if s > 0 else cw[::-1])
        return out


def transform(shift):
    """Column-major mat4: one path unit = one pixel, the path origin at the frame's centre + (shift, 0) pixels. All entries exact in binary32."""
    m = np.zeros(16, dtype=np.float32)
    m[0] = m[5] = 2.0 / SIZE
    m[10] = m[15] = 1.0
    m[12] = 2.0 * shift / SIZE
    assert float(m[12]) * SIZE / 2.0 == shift
    return m


def sample_x(msaa):
    """-> [SIZE, msaa] x positions of a row's samples."""
    return np.arange(SIZE, dtype=np.float64)[:, None] + SAMPLE_X[msaa][None, :]


def counts(stack, msaa, shift=None):
    """-> [SIZE, msaa] winding numbers of a row's samples (every row of the frame is the same), exact integers."""
    lefts = stack.lefts(shift)
    assert lefts.max() < RIGHT + (stack.shift if shift is None else shift) and (RIGHT + (stack.shift if shift is None else shift)) > SIZE
    order = np.argsort(lefts, kind="stable")
    sorted_lefts = lefts[order]
    prefix = np.concatenate([[0], np.cumsum(stack.signs[order])])
    x = sample_x(msaa)
    at = np.searchsorted(sorted_lefts, x, side="left")
    on_an_edge = np.isin(x, sorted_lefts)
    assert not on_an_edge.any(), "a sample on an edge: the excluded near-boundary samples of these scenes are zero by construction"
    return prefix[at]


def covered(stack, msaa, bits, shift=None):
    return np.mod(counts(stack, msaa, shift), 1 << bits) != 0


def image(stacks, msaa, bits, shifts=None):
    """Float64 premultiplied 'over' of the stacks in draw order, resolved -> ([SIZE, SIZE, 4] in [0, 1], translucent layers per pixel at
    most). An opaque source replaces (src + dst * 0)."""
    dst = np.zeros((SIZE, msaa, 4))
    translucent = np.zeros((SIZE, msaa), dtype=np.int64)
    for k, st in enumerate(stacks):
        cov = covered(st, msaa, bits, None if shifts is None else shifts[k])
        c = np.float64(np.float32(st.color))
        src = np.array([c[0] * c[3], c[1] * c[3], c[2] * c[3], c[3]])
        dst = np.where(cov[..., None], src + dst * (1.0 - src[3]), dst)
        translucent = np.where(cov, 0 if c[3] == 1.0 else translucent + 1, translucent)
    row = dst.mean(axis=1)
    return np.broadcast_to(row[None, :, :], (SIZE, SIZE, 4)), int(translucent.max())
