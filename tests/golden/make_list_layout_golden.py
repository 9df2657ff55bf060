"""Digests of the host blocks of the five record-driven list passes (driver_list, resize_list, resized_crop_list,
preprocess_list, background_list) on one seeded corpus per pass: tests/golden/list_layout_digests.json.

The layouts are pure host code whose whole result is a byte block, so a digest pins them: tests/test_list_layout_golden.py
rebuilds every block with the library under test and compares.  The file is generated ONCE, with the library the host
halves are to stay equal to; a differing byte afterwards is a defect of the library, not a reason to run this again.

    python tests/golden/make_list_layout_golden.py          (IMGXF_LIBRARY selects the library; no IMGXF_* knob set)

`corpus()` and `digests()` are what the test imports; nothing here touches a device."""
import hashlib
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
PATH = os.path.join(HERE, "list_layout_digests.json")
SEED = 20261021
N = 1024
SIDE = 520                                                  # sizes run from 1 x 1 up to SIDE per side
BUDGETS = (65536, 20000, 3000)                              # driver_list's LDS budgets
FILTERS = {"LANCZOS": 1, "BILINEAR": 2, "BICUBIC": 3, "BOX": 4}
CROP_SIZES = ((224, 224), (7, 5))                           # resized_crop_list's (Sh, Sw)
RESIZE, CROP = 256, 224                                     # preprocess_list's Resize and CenterCrop
DRIVER_TYPES = (0, 1, 2, 3, 4, 5, 6, 7, 8, 10, 12, 13)     # the codes of driver_list.TYPES and BLUR_FIXED
N_TALL, N_ONE, N_REPEAT = 32, 32, 160


def sha(a) -> str:
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def corpus() -> dict:
    """The geometry arrays of every pass, from one RandomState: frames of 1 .. SIDE per side, a fifth of them with
    fewer than 9 rows; boxes of one pixel and boxes more than 100 times as tall as wide; the last N_REPEAT entries
    repeat earlier ones, so tables are shared."""
    rs = np.random.RandomState(SEED)
    h, w = rs.randint(1, SIDE + 1, N), rs.randint(1, SIDE + 1, N)
    small = rs.rand(N) < 0.2
    h[small] = rs.randint(1, 9, small.sum())
    h[0], w[0], h[1], w[1] = 1, 1, SIDE, SIDE                # both ends of the range
    bh = np.minimum((rs.rand(N) * h).astype(int) + 1, h)
    bw = np.minimum((rs.rand(N) * w).astype(int) + 1, w)
    tall = np.arange(8, 8 + N_TALL)                          # a box of the `tall` route: bh > 100 bw, and rows are lost
    h[tall] = rs.randint(450, SIDE + 1, N_TALL)
    bh[tall], bw[tall] = h[tall], np.minimum(rs.randint(1, 5, N_TALL), w[tall])
    one = np.arange(8 + N_TALL, 8 + N_TALL + N_ONE)          # a box of one pixel
    bh[one], bw[one] = 1, 1
    top, left = (rs.rand(N) * (h - bh + 1)).astype(int), (rs.rand(N) * (w - bw + 1)).astype(int)
    oh, ow = rs.randint(1, 300, N), rs.randint(1, 300, N)
    ow[::3] = (ow[::3] + 3) // 4 * 4                         # widths that are multiples of 4, and widths that are not
    flip = rs.randint(0, 2, N)
    colour = rs.randint(0, 256, (N, 3))

    # driver_list: every type's parameters drawn so that most entries are accepted, and every refusal occurs
    types = np.array(DRIVER_TYPES)[rs.randint(0, len(DRIVER_TYPES), N)]
    types[rs.rand(N) < 0.02] = 9                             # 9 and 11 are no type
    types[rs.rand(N) < 0.01] = 11
    p = rs.uniform(-2, 2, (N, 2))
    m = types == 0
    p[m, 0] = rs.uniform(0.3, 2.2, m.sum())
    p[m & (rs.rand(N) < 0.1), 0] = 1.0
    p[m & (rs.rand(N) < 0.05), 0] = 0.0005                   # int(w s) below 1: refused for its size
    m = types == 1
    p[m, 0] = rs.uniform(-400, 400, m.sum())
    p[m & (rs.rand(N) < 0.1), 0] = 180.0                     # a turn
    p[m & (rs.rand(N) < 0.05), 0] = 0.0                      # a copy
    m = (types == 2) | (types == 3)
    p[m, 0] = rs.uniform(0.2, 1.8, m.sum())
    m = types == 4
    p[m, 0] = rs.uniform(-0.5, 0.5, m.sum())
    m = types == 5
    p[m] = rs.uniform(-400, 400, (m.sum(), 2))
    m = types == 8                                           # a corner that keeps the int(0.78 w) window inside, mostly
    cs = (0.78 * w).astype(int)
    p[m, 0] = np.floor(rs.rand(N) * (w - cs + 1))[m]
    p[m, 1] = np.floor(rs.rand(N) * (np.maximum(h - cs, 0) + 1))[m]
    m = (types == 12) | (types == 13)
    p[m, 0] = 2 * rs.randint(0, 16, m.sum()) + 1
    p[m, 1] = 0.5 * rs.randint(1, 11, m.sum())
    p[m & (rs.rand(N) < 0.05), 0] = 0.0                      # no blur: the drivers hand back the input
    chan = np.full(N, 3)
    chan[rs.rand(N) < 0.02] = 4                              # refused for its format
    frame = rs.randint(0, 64, N)

    src = rs.randint(0, N - N_REPEAT, N_REPEAT)              # repeated geometries
    for a in (h, w, bh, bw, top, left, oh, ow, flip, types, chan, frame):
        a[N - N_REPEAT:] = a[src]
    p[N - N_REPEAT:] = p[src]
    colour[N - N_REPEAT:] = colour[src]

    from imagetransformations_amd import tensor_maps as TM
    return {
        "driver_list": (np.stack([frame, types, h, w, chan], 1).astype(np.int32), p),
        "resize_list": np.stack([h, w, top, left, bh, bw, oh, ow], 1).astype(np.int32),
        "resized_crop_list": np.stack([h, w, top, left, bh, bw, flip], 1).astype(np.int32),
        "preprocess_list": TM.preprocess_geometry(list(zip(h.tolist(), w.tolist())), RESIZE, CROP),
        "background_list": np.stack([h, w, colour[:, 0], colour[:, 1], colour[:, 2]], 1).astype(np.int32),
    }


def _block(block) -> dict:
    return {"bytes": int(block.nbytes), "sha256": sha(block)}


def _driver(lay) -> dict:
    d = _block(lay["block"])
    d.update({k: sha(lay[k]) for k in ("out_off", "out_hw", "status")})
    d.update(out_bytes=lay["out_bytes"], lds_bytes=lay["lds_bytes"])
    return d


def layouts(c: dict):
    """(key, thunk) of every pass and parameter set, n = 0 included; a thunk lays out and returns what `digests` hashes
    (driver_list: the layout dict, else the block)."""
    from imagetransformations_amd import background_list as BG, driver_list as DL, resize_list as RL, tensor_maps as TM
    geo, p = c["driver_list"]
    for n, tag in ((N, ""), (0, "/n0")):
        for budget in (BUDGETS if n else BUDGETS[:1]):
            yield f"driver_list/{budget}{tag}", lambda n=n, budget=budget: DL.layout(geo[:n], p[:n], budget)
        for name in (("BILINEAR", "BICUBIC", "LANCZOS") if n else ("BICUBIC",)):
            f = FILTERS[name]
            yield f"resize_list/{name}{tag}", lambda n=n, f=f: RL.layout(c["resize_list"][:n], f)
            yield f"preprocess_list/{name}{tag}", lambda n=n, f=f: TM.preprocess_layout(c["preprocess_list"][:n], CROP,
                                                                                       interpolation=f)
        for name in (("BILINEAR", "BICUBIC", "BOX") if n else ("BICUBIC",)):
            for size in (CROP_SIZES if n else CROP_SIZES[:1]):
                yield (f"resized_crop_list/{name}/{size[0]}x{size[1]}{tag}",
                       lambda n=n, name=name, size=size: TM.resized_crop_layout(c["resized_crop_list"][:n], size,
                                                                                interpolation=FILTERS[name]))
        yield f"background_list{tag}", lambda n=n: BG.layout(c["background_list"][:n])


def digests(c: dict) -> dict:
    out = {}
    for key, make in layouts(c):
        made = make()
        out[key] = _driver(made) if key.startswith("driver_list") else _block(made)
    return out


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
    if any(k.startswith("IMGXF_") and k != "IMGXF_LIBRARY" for k in os.environ):
        sys.exit("an IMGXF_* knob is set: the float blur's route (and so a status) depends on them")
    d = digests(corpus())
    with open(PATH, "w") as f:
        json.dump(d, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"{len(d)} digests -> {PATH}")
