"""The numpy model of crh_image_crop, crh_image_create_from_frame_region and crh_image_statistics (include/contrast_hip.h states the
rules), shared by tests/test_regions_cpu.py and tests/test_gpu_regions.py: the crop by padded slicing, the histogram by np.bincount per
channel, the bounds from np.nonzero. Nothing here calls the library."""
import numpy as np

R, G, B, A = 0, 1, 2, 3
INT32_MIN, INT32_MAX = -2 ** 31, 2 ** 31 - 1


def crop(src, x, y, width, height):
    """-> the (height, width, 4) uint8 result: texel (i, j) is src's texel (x + i, y + j), zeros outside src; x and y any integers."""
    h, w = src.shape[:2]
    out = np.zeros((height, width, 4), dtype=np.uint8)
    # the part of the source the rectangle holds, [sx0, sx1) x [sy0, sy1), in Python's unbounded integers
    sx0, sy0, sx1, sy1 = max(x, 0), max(y, 0), min(x + width, w), min(y + height, h)
    if sx0 < sx1 and sy0 < sy1:
        out[sy0 - y:sy1 - y, sx0 - x:sx1 - x] = src[sy0:sy1, sx0:sx1]
    return out


def statistics(src, channel=A, threshold=1):
    """-> (histogram, bounds, count): a (4, 256) uint32 array of how many texels store each code in each channel, (x0, y0, x1, y1)
    half-open around the texels whose stored code of `channel` is >= threshold ((0, 0, 0, 0) if none is), and their number."""
    histogram = np.stack([np.bincount(src[..., c].reshape(-1), minlength=256) for c in range(4)]).astype(np.uint32)
    rows, columns = np.nonzero(src[..., channel] >= threshold)
    if rows.size == 0:
        return histogram, (0, 0, 0, 0), 0
    return histogram, (int(columns.min()), int(rows.min()), int(columns.max()) + 1, int(rows.max()) + 1), int(rows.size)


def random_texels(w, h, seed, premultiplied=True):
    rng = np.random.default_rng(seed)
    src = rng.integers(0, 256, (h, w, 4), dtype=np.uint8)
    if premultiplied:
        src[..., :3] = np.minimum(src[..., :3], src[..., 3:])
    return src


def rectangles(w, h):
    """The classes of crop rectangle against a w x h source, as (name, x, y, width, height): inside, over each side and each corner,
    containing the source, missing it on each side, and with x and y at the int32 extremes."""
    a, b = max(1, w // 2), max(1, h // 2)
    cases = [("inside", w // 4, h // 4, a, b), ("whole", 0, 0, w, h),
             ("left", -2, h // 4, a, b), ("right", w - a + 2, h // 4, a, b), ("top", w // 4, -3, a, b), ("bottom", w // 4, h - b + 1, a, b),
             ("top-left", -2, -3, a, b), ("top-right", w - a + 2, -3, a, b), ("bottom-left", -2, h - b + 1, a, b), ("bottom-right", w - a + 2, h - b + 1, a, b),
             ("contains", -3, -2, w + 7, h + 5),
             ("misses-left", -a - 1, 0, a, b), ("misses-right", w, 0, a, b), ("misses-top", 0, -b, a, b), ("misses-bottom", 0, h + 4, a, b),
             ("touches-left", -a + 1, 0, a, b),
             ("x-min", INT32_MIN, 0, a, b), ("x-max", INT32_MAX, 0, a, b), ("y-min", 0, INT32_MIN, a, b), ("y-max", 0, INT32_MAX, a, b),
             ("both-min", INT32_MIN, INT32_MIN, a, b), ("both-max", INT32_MAX, INT32_MAX, a, b)]
    return cases
