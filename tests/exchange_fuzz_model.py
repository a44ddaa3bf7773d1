"""The generator and the host model of the stateful exchange fuzz (tests/test_gpu_exchange_fuzz.py): random op sequences over one Renderer, a
pool of ten frames in two sizes and both layer formats, and two loopback groups (world 3 and world 5) that live for the whole sequence, so
that geometry and format change under them and frames change role: a layer becomes a result, a result a layer of the other group, at any
rank, with nothing in between that would wait for the exchange that wrote it.

The generator keeps the STRUCTURE of every frame (what wrote it last, its tile rows, whether it is a result nobody has looked at); the Model
keeps the BYTES: an upload's are the op's, a pass's are the download taken right after it (the renderer is not what this fuzz checks), and a
result's come from exchange_model alone — a result frame is not downloaded before it has served as a layer (the last results of a sequence
apart, which nothing follows). No GPU and no library call in here."""
import numpy as np

import exchange_model as M

RGBA8, RGBA16F = 0, 1
FRAMES = ((0, RGBA8), (0, RGBA8), (0, RGBA8), (0, RGBA8), (0, RGBA16F), (0, RGBA16F), (1, RGBA8), (1, RGBA8), (1, RGBA8), (1, RGBA16F))  # (size index, format)
WORLDS = (3, 5)  # group 0 and group 1
KINDS = ("upload", "clear", "render", "render_over", "set_rows", "exchange", "gather", "download")
CHOICES = ("upload", "clear", "render", "render_over", "rows_render", "exchange", "gather", "download")
WEIGHTS = (0.14, 0.04, 0.12, 0.06, 0.06, 0.40, 0.06, 0.12)


def slab_rows(height, world):
    tiles = (height + 15) // 16
    out = []
    for r in range(world):
        b, e = M.slab_tiles(1, tiles, r, world)
        out.append((min(b * 16, height), min(e * 16, height)))
    return out


def sparse_bytes(rng, w, h):
    """An upload: some tiles, some of their pixels; premultiplied bytes, raw bytes (colour above alpha) or colour under alpha 0."""
    tx, ty = M.tile_grid(w, h)
    tiles = rng.uniform(size=tx * ty) < float(rng.choice([0.1, 0.4, 1.0]))
    mask = M.tile_pixels(tiles, w, h) & (rng.uniform(size=(h, w)) < float(rng.choice([0.02, 0.5, 1.0])))
    how = int(rng.randint(0, 3))
    pixels = M.random_premultiplied(rng, w, h) if how == 0 else rng.randint(0, 256, (h, w, 4)).astype(np.uint8)
    if how == 2:
        pixels[..., 3] = 0
    return pixels * mask[..., None].astype(np.uint8)


def random_scene(rng, w, h):
    """Four to seven rectangles, one Shape each, some on pixel edges and some not, straight colours with a share of opaque ones."""
    n = int(rng.randint(4, 8))
    rects = []
    for i in range(n):
        x0, y0 = rng.uniform(-4, w - 4), rng.uniform(-4, h - 4)
        x1, y1 = x0 + rng.uniform(2, w / 2.0), y0 + rng.uniform(2, h / 2.0)
        r = (x0, y0, x1, y1)
        rects.append(tuple(float(np.floor(v)) for v in r) if i % 2 == 0 else tuple(float(np.float32(v)) for v in r))
    colors = np.concatenate([rng.uniform(0, 1, (n, 3)), rng.uniform(0.2, 1, (n, 1))], axis=1).astype(np.float32)
    colors[::3, 3] = 1.0
    return dict(rects=rects, colors=colors)


def generate(seed):
    """-> (setup, ops). Every op holds all the replay needs; exchange and gather ops carry the facts the coverage conditions count."""
    rng = np.random.RandomState(8800 + seed)
    sizes = [(int(rng.randint(60, 201)), int(rng.randint(50, 137))), (int(rng.randint(20, 121)), int(rng.randint(17, 33)))]  # the second: two tile rows for 3 and 5 ranks
    setup = dict(seed=seed, sizes=sizes, msaa=int(rng.choice([1, 4])), scenes=[[random_scene(rng, *size) for _ in range(2)] for size in sizes])
    frames = [dict(size=s, format=f, state="clear", rows=None, pending=False, served=False, writer=None) for s, f in FRAMES]
    last = [None, None]  # (size index, format) of each group's last exchange that went through
    ops = []

    def of(size, fmt=None):
        return [j for j, f in enumerate(frames) if f["size"] == size and (fmt is None or f["format"] == fmt)]

    def pick(items):
        return items[int(rng.randint(0, len(items)))]

    def written(j, state):
        frames[j].update(state=state, pending=False, served=False, writer=None)

    def whole_rows(j):
        if frames[j]["rows"] is not None:
            ops.append(dict(kind="set_rows", frame=j, rows=(0, sizes[frames[j]["size"]][1])))
            frames[j]["rows"] = None
            written(j, "clear")

    def render(j, over):
        ops.append(dict(kind="render_over" if over else "render", frame=j, scene=int(rng.randint(0, 2)), after=frames[j]["state"]))
        written(j, "render")

    def exchange(g, layers, result, fails, why):
        s, fmt = frames[layers[0]]["size"], frames[layers[0]]["format"]
        op = dict(kind="exchange", group=g, layers=layers, result=result, fails=fails, why=why, scan=bool(rng.uniform() < 0.5))
        if not fails:
            h = sizes[s][1]
            op["result_as_layer"] = sum(1 for k, j in enumerate(layers) if k >= 1 and frames[j]["pending"] and j not in layers[1:k])
            op["after_other_group"] = bool(frames[result]["pending"] and frames[result]["writer"] == 1 - g)
            op["size_changed"] = bool(last[g] is not None and last[g][0] != s)
            op["format_changed"] = bool(last[g] is not None and last[g][1] != fmt)
            op["empty_slabs"] = max(0, WORLDS[g] - (h + 15) // 16)
            op["aliased"] = result in layers
            last[g] = (s, fmt)
            for j in layers:
                if frames[j]["pending"]:
                    frames[j]["served"] = True
            frames[result].update(state="result", pending=True, served=False, writer=g)
        ops.append(op)

    n_steps = int(rng.randint(28, 40))
    ops.append(dict(kind="upload", frame=0, pixels=sparse_bytes(rng, *sizes[0])))
    written(0, "upload")
    while len(ops) < n_steps:
        choice = CHOICES[int(rng.choice(len(CHOICES), p=np.float64(WEIGHTS) / np.sum(WEIGHTS)))]
        j = int(rng.randint(0, len(frames)))
        f = frames[j]
        if choice == "upload":
            if f["format"] != RGBA8:
                continue
            whole_rows(j)
            ops.append(dict(kind="upload", frame=j, pixels=sparse_bytes(rng, *sizes[f["size"]])))
            written(j, "upload")
        elif choice == "clear":
            ops.append(dict(kind="clear", frame=j))
            written(j, "clear")
        elif choice == "render":
            if f["state"] != "clear":
                ops.append(dict(kind="clear", frame=j))
                written(j, "clear")
            render(j, False)
        elif choice == "render_over":
            if f["state"] == "clear" or f["pending"]:  # (a pass over a result nobody has looked at would take the result out of the model's hands)
                continue
            render(j, True)
        elif choice == "rows_render":
            h = sizes[f["size"]][1]
            tiles = (h + 15) // 16
            t0 = int(rng.randint(0, tiles))
            t1 = int(rng.randint(t0 + 1, tiles + 1))
            rows = (t0 * 16, min(h, t1 * 16))
            ops.append(dict(kind="set_rows", frame=j, rows=rows))
            f["rows"] = None if rows == (0, h) else rows
            written(j, "clear")
            render(j, False)
        elif choice == "exchange":
            g = int(rng.randint(0, 2))
            world = WORLDS[g]
            s = int(rng.uniform() < 0.4)
            fmt = RGBA16F if rng.uniform() < 0.25 else RGBA8
            pool = of(s, fmt)
            waiting = [k for k in of(s, RGBA8) if frames[k]["pending"]] if fmt == RGBA8 else []
            layers = [pick(waiting) if waiting and k >= 1 and rng.uniform() < 0.6 else pick(pool) for k in range(world)]
            results = of(s, RGBA8)
            result = pick(results)
            how = rng.uniform()
            if how < 0.07:
                layers[int(rng.randint(0, world))] = pick(of(1 - s, fmt))
                exchange(g, layers, result, True, "sizes")
            elif how < 0.12:
                k = int(rng.randint(0, world))
                others = [c for c in of(s, 1 - fmt)]
                layers = [pick(pool) for _ in range(world)]
                layers[k] = pick(others)
                if len({frames[c]["format"] for c in layers}) < 2:
                    continue
                exchange(g, layers, result, True, "formats")
            elif how < 0.17:
                exchange(g, layers, pick(of(s, RGBA16F)), True, "a 16F result")
            else:
                whole_rows(result)
                exchange(g, layers, result, False, None)
        elif choice == "gather":
            g = int(rng.randint(0, 2))
            world = WORLDS[g]
            s = int(rng.uniform() < 0.5)
            h = sizes[s][1]
            rows = slab_rows(h, world)
            busy = [r for r in rows if r[1] > r[0]]
            pool = of(s, RGBA8)
            if len(busy) + 1 > len(pool):
                continue
            chosen = [int(v) for v in rng.permutation(pool)[:len(busy) + 1]]
            result, layers = chosen[0], chosen[1:] + [chosen[1]] * (world - len(busy))  # (a rank without rows takes no part: any frame does)
            for k, r in enumerate(busy):
                ops.append(dict(kind="set_rows", frame=layers[k], rows=r))
                frames[layers[k]]["rows"] = None if r == (0, h) else r
                written(layers[k], "clear")
                render(layers[k], False)
            whole_rows(result)
            ops.append(dict(kind="gather", group=g, layers=layers, result=result, after_other_group=bool(frames[result]["pending"] and frames[result]["writer"] == 1 - g),
                            empty_slabs=world - len(busy)))
            frames[result].update(state="result", pending=True, served=False, writer=g)
        else:
            assert choice == "download"
            if f["pending"] and not f["served"]:
                continue
            ops.append(dict(kind="download", frame=j, what=f["state"], served=bool(f["pending"])))
            f.update(pending=False, served=False)
    # the results nobody has looked at serve as layers of one last exchange per size, then everything is compared
    for s in (0, 1):
        waiting = [k for k in of(s, RGBA8) if frames[k]["pending"] and not frames[k]["served"]]
        if waiting:
            g = s
            layers = [waiting[k % len(waiting)] if k >= 1 else pick(of(s, RGBA8)) for k in range(WORLDS[g])]
            result = pick(of(s, RGBA8))
            whole_rows(result)
            exchange(g, layers, result, False, None)
    for j, f in enumerate(frames):
        ops.append(dict(kind="download", frame=j, what=f["state"], served=bool(f["pending"] and f["served"]), final=True))
    return setup, ops


class Model:
    """The bytes every frame must hold. apply(op, observed) -> what the device's answer to the op is compared with: the image of a download,
    dict(image=None, traffic=[...]) for an exchange that goes through (the traffic is the pixel-scan path's), None otherwise. `observed` = the
    download taken right after a pass, which becomes the frame's bytes."""

    def __init__(self, setup):
        self.sizes = setup["sizes"]
        self.bytes = [np.zeros((self.sizes[s][1], self.sizes[s][0], 4), dtype=np.float16 if f == RGBA16F else np.uint8) for s, f in FRAMES]

    def must_fail(self, op):
        """An exchange is refused when its layers differ in size or format or its result is not an RGBA8 frame of their size."""
        kinds = {FRAMES[j] for j in op["layers"]}
        return len(kinds) != 1 or FRAMES[op["result"]] != (FRAMES[op["layers"][0]][0], RGBA8)

    def apply(self, op, observed=None):
        kind = op["kind"]
        if kind == "upload":
            self.bytes[op["frame"]] = op["pixels"]
        elif kind in ("clear", "set_rows"):
            self.bytes[op["frame"]] = np.zeros_like(self.bytes[op["frame"]])
        elif kind in ("render", "render_over"):
            assert observed is not None and observed.shape == self.bytes[op["frame"]].shape and observed.dtype == self.bytes[op["frame"]].dtype
            self.bytes[op["frame"]] = observed
        elif kind == "exchange":
            assert self.must_fail(op) == op["fails"]
            if op["fails"]:
                return None
            layers = np.stack([self.bytes[j] for j in op["layers"]])
            self.bytes[op["result"]] = M.composite(layers)
            return dict(traffic=M.traffic_of_layers(layers))
        elif kind == "gather":
            height = self.bytes[op["result"]].shape[0]
            self.bytes[op["result"]] = M.gather_slabs([self.bytes[j] for j in op["layers"]], height, len(op["layers"]))
        elif kind == "download":
            return self.bytes[op["frame"]]
        else:
            raise AssertionError(kind)
        return None
