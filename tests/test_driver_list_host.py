"""Host half of driver_list.apply_list (imgxf_driver_list_layout_host): the block it lays out for twelve entries over six
small sizes — work units, output offsets, shear's width, Lanczos tables and their sharing, refusals.  No device."""
import ctypes
import math

import numpy as np
import pytest

from oracle import imgxf_oracle as O

SIZES = [(1, 1), (2, 3), (7, 5), (10, 10), (37, 61), (61, 37)]          # (h, w); frame index = position
# (frame, type, args)
ENTRIES = [
    (4, 'scale', (1.3,)), (5, 'scale', (0.9,)), (4, 'scale', (1.3,)),  # 0 and 2: equal geometry
    (3, 'scale', (1.0,)), (2, 'scale', (1.1,)),                          # factor 1; int(5 * 1.1) == 5
    (0, 'scale', (0.9,)),                                                # resized size 0: refused
    (3, 'rotation', (90.0,)),                                            # transpose on a square frame: refused
    (1, 'rotation', (22.5,)), (4, 'shear', (0.30000000000000004,)), (5, 'translation', (5, -45)),
    (2, 'lighten_darken', (-0.05,)), (0, 'gaussian_noise', (None,)),
]
REFUSED = {5: 2, 6: 3}                                                   # entry -> status (SIZE, TURN)


def _dl():
    from imagetransformations_amd import driver_list
    return driver_list


def _layout(entries, sizes=SIZES, lds_bytes=None):
    dl = _dl()
    geo = [(f, dl.TYPES[t], sizes[f][0], sizes[f][1], 3) for f, t, _ in entries]
    par = [dl.entry_params(t, a) for _, t, a in entries]
    return dl.layout(geo, par, dl.DRIVER_LIST_LDS_BYTES if lds_bytes is None else lds_bytes)


def _window_tables(in_size, s):
    """(bounds, coefficients) of oracle.lanczos_coeffs for in -> int(in * s), sliced to the centre-crop window above 1."""
    out = int(in_size * s)
    b, k, _ = O.lanczos_coeffs(in_size, out)
    if s > 1.0:
        first = (out - in_size) // 2
        b, k = b[first:first + in_size], k[first:first + in_size]
    return b, k


def test_units_offsets_tables_and_refusals():
    dl = _dl()
    lay = _layout(ENTRIES)
    block, status, out_off, out_hw = lay["block"], lay["status"], lay["out_off"], lay["out_hw"]
    hd, rec, units = dl.block_views(block)
    words = block.view(np.int32)
    assert hd["n_entries"] == len(ENTRIES) and hd["total_bytes"] == block.nbytes
    assert hd["lds_bytes"] == lay["lds_bytes"] <= dl.DRIVER_LIST_LDS_BYTES
    assert status.tolist() == [REFUSED.get(j, 0) for j in range(len(ENTRIES))]
    assert np.array_equal(rec["status"], status) and np.array_equal(rec["out_off"], out_off)
    spans = []
    for j, (f, t, args) in enumerate(ENTRIES):
        h, w = SIZES[f]
        mine = units[units["entry"] == j]
        if j in REFUSED:
            assert out_off[j] == -1 and len(mine) == 0
            continue
        oh, ow = out_hw[j]
        assert (oh, ow) == ((h, w + math.ceil(args[0] * h)) if t == 'shear' else (h, w))
        # the units cover the output rows exactly once, in order
        assert mine["y0"].tolist()[0] == 0 and (mine["y0"] + mine["ny"]).tolist() == mine["y0"].tolist()[1:] + [oh]
        assert np.all(mine["ny"] >= 1)
        assert out_off[j] % 16 == 0 and out_off[j] % 48 == 0       # 16-byte aligned, and whole pixels into the block
        spans.append((int(out_off[j]), int(out_off[j]) + int(oh) * int(ow) * 3))
        is_scale = t == 'scale'
        assert np.all((np.flatnonzero(units["entry"] == j) >= hd["n_plain"]) == is_scale)      # scale units: second launch
        if is_scale:
            r, s = rec[j], args[0]
            bx, kx = _window_tables(w, s)
            by, ky = _window_tables(h, s)
            assert (r["win_w"], r["win_h"]) == (len(bx), len(by)) and (r["ksx"], r["ksy"]) == (kx.shape[1], ky.shape[1])
            assert np.array_equal(words[r["bounds_x"]:r["bounds_x"] + 2 * len(bx)].reshape(-1, 2), bx)
            assert np.array_equal(words[r["coeffs_x"]:r["coeffs_x"] + kx.size].reshape(kx.shape), kx)
            assert np.array_equal(words[r["bounds_y"]:r["bounds_y"] + 2 * len(by)].reshape(-1, 2), by)
            assert np.array_equal(words[r["coeffs_y"]:r["coeffs_y"] + ky.size].reshape(ky.shape), ky)
            nw, nh, mode, ox, oy = O.scale_geometry(w, h, s)
            assert (r["win_left"], r["win_top"]) == ((ox, oy) if mode == "paste" else (0, 0))
            assert r["row0"] == by[:, 0].min() and r["row0"] + r["nrows"] == by.sum(1).max() <= h
            assert r["col0"] == bx[:, 0].min() and r["col0"] + r["ncols"] == bx.sum(1).max() <= w
            assert np.all(mine["lds_bytes"] <= hd["lds_bytes"])
    spans.sort()
    assert all(a1 <= b0 for (_, a1), (b0, _) in zip(spans, spans[1:]))   # the outputs do not overlap
    assert spans[-1][1] <= lay["out_bytes"] == hd["out_bytes"]
    # two entries of equal geometry share their tables; the others have their own
    keys = ("bounds_x", "coeffs_x", "bounds_y", "coeffs_y")
    assert all(rec[0][k] == rec[2][k] for k in keys)
    assert len({int(rec[j]["bounds_x"]) for j in (0, 1, 3, 4)}) == 4
    # the 37 x 61 and 61 x 37 frames share nothing here, but one axis table serves both axes of a square frame
    assert rec[3]["bounds_x"] == rec[3]["bounds_y"]


def test_rotation_matrix_and_copy():
    """The record's 16.16 coefficients are affine_fixed's of ops.rotate_matrix; angle 0 is stated as a copy."""
    dl = _dl()
    ents = [(1, 'rotation', (22.5,)), (4, 'rotation', (-17.5,)), (3, 'rotation', (0.0,)), (5, 'rotation', (90.0,)),
            (3, 'rotation', (180.0,)), (3, 'rotation', (-90.0,))]
    lay = _layout(ents)
    _, rec, _ = dl.block_views(lay["block"])
    assert lay["status"].tolist() == [0, 0, 0, 0, 3, 3]
    for j in (0, 1, 3):
        h, w = SIZES[ents[j][0]]
        kind, m = O.rotate_plan(w, h, -ents[j][2][0])
        assert kind == "affine"
        fx = [O._fix16(m[0]), O._fix16(m[1]), O._fix16(m[2] + m[0] * 0.5 + m[1] * 0.5),
              O._fix16(m[3]), O._fix16(m[4]), O._fix16(m[5] + m[3] * 0.5 + m[4] * 0.5)]
        assert rec[j]["fx"].tolist() == fx and rec[j]["op"] == dl.TYPES['rotation']
    assert rec[2]["op"] == dl.TYPES['translation'] and (rec[2]["dx"], rec[2]["dy"]) == (0, 0)


def test_small_budget_refuses_the_scale_alone():
    """A 64 x 48 scale whose single row does not fit the budget is refused; the other entries keep status ok."""
    dl = _dl()
    sizes = [(64, 48)]
    ents = [(0, 'scale', (1.3,)), (0, 'scale', (0.9,)), (0, 'contrast', (0.5,)), (0, 'shear', (1.0,))]
    # one output row at factor 1.3: 7 touched rows x 12 * ceil(48 / 4) = 1008 bytes + staging
    lay = _layout(ents, sizes, lds_bytes=1000)
    assert lay["status"].tolist() == [dl.REFUSED_LDS, dl.REFUSED_LDS, dl.OK, dl.OK]
    hd, _, units = dl.block_views(lay["block"])
    assert hd["n_plain"] == hd["n_units"] == len(units) and hd["lds_bytes"] == 0
    assert _layout(ents, sizes)["status"].tolist() == [0, 0, 0, 0]


def test_format_refusal_and_argument_errors():
    from imagetransformations_amd import _ffi
    dl = _dl()
    lay = dl.layout([(0, 0, 8, 8, 1), (0, 3, 8, 8, 0), (0, 3, 8, 8, 3), (0, 9, 8, 8, 3)], [(1.1, 0)] * 4)
    assert lay["status"].tolist() == [dl.REFUSED_FORMAT, dl.REFUSED_FORMAT, dl.OK, dl.REFUSED_OTHER]
    fn = _ffi.lib.imgxf_driver_list_layout_host
    geo = np.array([[0, 0, 37, 61, 3]], np.int32)
    par = np.array([[1.3, 0.0]], np.float64)
    need = ctypes.c_size_t(0)
    gp, pp, np_ = geo.ctypes.data, par.ctypes.data, ctypes.byref(need)
    assert fn(None, pp, 1, 65536, None, 0, np_, None, None, None, None, None) == _ffi.ERR_NULL
    assert fn(gp, pp, 1, 65536, None, 0, None, None, None, None, None, None) == _ffi.ERR_NULL
    assert fn(gp, pp, -1, 65536, None, 0, np_, None, None, None, None, None) == _ffi.ERR_ARG
    assert fn(gp, pp, 1, 0, None, 0, np_, None, None, None, None, None) == _ffi.ERR_ARG
    assert fn(gp, pp, 1, 65536, None, 0, np_, None, None, None, None, None) == _ffi.OK and need.value > 0
    buf = np.zeros(need.value, np.uint8)
    assert fn(gp, pp, 1, 65536, buf.ctypes.data, need.value - 1, np_, None, None, None, None, None) == _ffi.ERR_WORKSPACE
    assert fn(gp, pp, 1, 65536, buf.ctypes.data, need.value, np_, None, None, None, None, None) == _ffi.OK
    assert fn(None, None, 0, 65536, None, 0, np_, None, None, None, None, None) == _ffi.OK and need.value == 48
    assert _ffi.lib.imgxf_driver_list_u8(None, None, None, 0, None) == _ffi.ERR_NULL
    assert _ffi.lib.imgxf_driver_list_u8(buf.ctypes.data, None, None, 0, None) == _ffi.ERR_NULL


@pytest.mark.parametrize("s", [0.9, 1.0, 1.1, 1.2000000000000002, 1.3])
def test_block_evaluated_in_numpy_equals_the_oracle(s):
    """The scale records, evaluated in NumPy as the kernel evaluates them (horizontal pass, uint8 intermediate, vertical
    pass, black canvas), give oracle.apply_scale."""
    dl = _dl()
    rng = np.random.default_rng(3)
    sizes = [(h, w) for h, w in SIZES if int(h * s) >= 1 and int(w * s) >= 1]
    lay = _layout([(i, 'scale', (s,)) for i in range(len(sizes))], sizes)
    _, rec, _ = dl.block_views(lay["block"])
    words = lay["block"].view(np.int32)
    assert not lay["status"].any()
    for (h, w), r in zip(sizes, rec):
        a = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)

        def axis(src, bounds, coeffs, count, ks):
            b = words[bounds:bounds + 2 * count].reshape(-1, 2)
            k = words[coeffs:coeffs + count * ks].reshape(count, ks).astype(np.int64)
            out = np.empty((count,) + src.shape[1:], np.uint8)
            for j in range(count):
                acc = (src[b[j, 0]:b[j, 0] + b[j, 1]].astype(np.int64) * k[j, :b[j, 1], None, None]).sum(0) + (1 << 21)
                out[j] = np.clip(acc >> 22, 0, 255)
            return out
        mid = axis(a.transpose(1, 0, 2), r["bounds_x"], r["coeffs_x"], r["win_w"], r["ksx"]).transpose(1, 0, 2)
        win = axis(mid, r["bounds_y"], r["coeffs_y"], r["win_h"], r["ksy"])
        got = np.zeros((r["oh"], r["ow"], 3), np.uint8)
        got[r["win_top"]:r["win_top"] + r["win_h"], r["win_left"]:r["win_left"] + r["win_w"]] = win
        assert np.array_equal(got, O.apply_scale(a, s)), (h, w, s)
