"""The guarded fp32 affine kernels on inputs where the guard decides: frames whose fp64 value lies
just below, just above or exactly on an integer for thousands of bytes (near_integer_corpus.py;
test_near_integer_corpus.py proves those properties on the reference alone).  Every bilinear route of
run_affine and every bicubic one must give Pillow's bytes on every frame of a batch; the fp32 mode and
the fp32 side output must stay inside the 1e-5 contract.

Each case first asserts which kernel the dispatcher takes for its geometry (`bilinear_route`, a
restatement of the box formulas and alignment tests of plan_affine in csrc/affine_route.h, kept in
affine_route.py): a change to those limits updates the function with it, and a geometry that silently
moves to another kernel fails here instead of leaving a kernel untested."""
import functools
import os

import numpy as np
import pytest
import torch

import near_integer_corpus as C
from affine_route import bicubic_route, bilinear_route
from oracle import imgxf_oracle as O
from test_gpu_parity import dev, host

pytestmark = pytest.mark.gpu

MATS = {**C.BILINEAR, **C.DYADIC}
PICK = {1: (0,), 3: (0, 7, 4), 5: (0, 7, 3, 10, 5), 12: tuple(range(12))}     # variants in a batch of n: plain and complemented mixed


@functools.lru_cache(maxsize=None)
def _variants(name, channel=None):
    v = C.variants(C.frame(name))
    return v if channel is None else np.ascontiguousarray(v[..., channel])


@functools.lru_cache(maxsize=None)
def _ref(kind, name, i, size, m, fill, channel=None):
    fn = O.affine_bicubic if kind == "bicubic" else O.affine_bilinear
    return fn(_variants(name, channel)[i], size, list(m), fill=fill)


@functools.lru_cache(maxsize=None)
def _ref_float(name, i, size, m, fill):
    return O.affine_bilinear(_variants(name)[i], size, list(m), fill=fill, return_float=True)


def _offset_view(a, byte_offset, device):
    """The batch `a` on the device in storage that starts `byte_offset` bytes after an aligned address."""
    buf = torch.zeros(a.size + 64, dtype=torch.uint8, device=device)
    assert buf.data_ptr() % 16 == 0
    v = buf[byte_offset:byte_offset + a.size].view(a.shape)
    v.copy_(torch.from_numpy(a))
    assert v.data_ptr() % 16 == byte_offset % 16
    return v


def _set_knobs(monkeypatch, knobs):
    for k in ("FPB", "NO_DMA", "NO_LDS", "NO_TALL", "NO_SHEAR_FAST"):
        if "IMGXF_AFFINE_" + k in os.environ:
            monkeypatch.delenv("IMGXF_AFFINE_" + k)
    for k, v in knobs.items():
        monkeypatch.setenv("IMGXF_AFFINE_" + k, str(v))


def _q(v):
    return np.clip(v, 0, 255).astype(np.int64).astype(np.uint8)


# (route, uses the list kernel, corpus, n, output size, knobs, fill, source byte offset)
W0, W1 = (160, 96), (150, 96)
BLACK, FILL = (0, 0, 0), (9, 8, 7)
# D1 (unit scale) cannot reach the batch kernels or the tall tiles: its 32 x 64 box is 67 rows (> 64) and its 32 x 16 box
# 35 pixels wide (> 28), so it runs through affine_bilinear_lds_kernel<49> at every batch and output size below, and
# D2 stands in for it as the all-ties frame of the wq / mf / interior rows.
CASES = [
    ("wq", False, "M1", 5, W0, {}, BLACK, 0), ("wq", False, "M1", 12, W0, {}, FILL, 0),
    ("wq", False, "D2", 5, W0, {}, BLACK, 0), ("wq", False, "D2", 12, W0, {}, BLACK, 0),
    ("wq", False, "M1", 5, W0, {"FPB": 2}, BLACK, 0), ("wq", False, "D2", 5, W0, {"FPB": 2}, BLACK, 0),
    ("mf13_dma", False, "M1", 5, W1, {"FPB": 2}, BLACK, 0), ("mf13_dma", False, "M1", 5, W1, {"FPB": 16}, FILL, 0),
    ("mf13_dma", False, "D2", 5, W1, {"FPB": 2}, BLACK, 0), ("mf13_dma", False, "D2", 5, W1, {"FPB": 16}, BLACK, 0),
    ("mf13", True, "M1", 5, W1, {"NO_DMA": 1, "FPB": 2}, BLACK, 0), ("mf13", True, "M1", 5, W1, {"NO_DMA": 1}, FILL, 0),
    ("mf13", True, "D2", 5, W1, {"NO_DMA": 1}, BLACK, 0), ("mf13", True, "M1", 5, W1, {}, BLACK, 4),
    ("mf16", True, "M2", 5, W0, {}, BLACK, 0),
    ("lds_interior", True, "M1", 1, W0, {}, BLACK, 0), ("lds_interior", True, "M2", 1, W0, {}, FILL, 0),
    ("lds_interior", True, "D2", 1, W0, {}, BLACK, 0),
    ("lds49", False, "M3", 1, W0, {}, BLACK, 0), ("lds49", False, "M3", 3, W0, {}, BLACK, 0),
    ("lds49", False, "M1", 3, W0, {"NO_TALL": 1}, BLACK, 0),
    ("lds49", False, "D1", 1, W0, {}, BLACK, 0), ("lds49", False, "D1", 5, W0, {}, BLACK, 0), ("lds49", False, "D1", 5, W1, {}, FILL, 0),
    ("lds65", False, "M4", 3, W0, {}, BLACK, 0), ("lds97", False, "M5", 3, W0, {}, BLACK, 0),
    ("global3", False, "M1", 3, W0, {"NO_LDS": 1}, BLACK, 0), ("global3", False, "D2", 3, W0, {"NO_LDS": 1}, BLACK, 0),
    ("global3", False, "D1", 3, W0, {"NO_LDS": 1}, BLACK, 0), ("global3", False, "M1", 3, W0, {}, BLACK, 1),
]


@pytest.mark.parametrize("route,lists,name,n,size,knobs,fill,offset", CASES,
                         ids=[f"{c[0]}-{c[2]}-n{c[3]}-{c[4][0]}-{'-'.join(f'{k}{v}' for k, v in c[5].items()) or 'default'}-fill{c[6][0]}-off{c[7]}" for c in CASES])
def test_bilinear_precise_equals_pillow(device, monkeypatch, route, lists, name, n, size, knobs, fill, offset):
    from imagetransformations_amd import ops
    _set_knobs(monkeypatch, knobs)
    m = tuple(MATS[name][0])
    for pick in ([(0,), (9,)] if n == 1 else [PICK[n]]):           # single frames: a plain and a complemented one
        a = _variants(name)[list(pick)]
        t = _offset_view(a, offset, device) if offset else dev(a, device)
        assert bilinear_route(t, m, size) == (route, lists)
        got = host(ops.affine(t, m, size, ops.BILINEAR, fill, precise=True))
        for j, i in enumerate(pick):
            want = _ref("bilinear", name, i, size, m, fill)
            assert np.array_equal(got[j], want), (name, i, int((got[j] != want).sum()))


def test_bilinear_every_other_frame_view(device, monkeypatch):
    """big[::2] (frame stride of two frames) through the LDS-DMA kernel."""
    from imagetransformations_amd import ops
    _set_knobs(monkeypatch, {})
    m = tuple(MATS["M1"][0])
    big = dev(_variants("M1")[:10], device)
    assert bilinear_route(big[::2], m, W1) == ("mf13_dma", False)
    got = host(ops.affine(big[::2], m, W1, ops.BILINEAR, BLACK, precise=True))
    for j in range(5):
        assert np.array_equal(got[j], _ref("bilinear", "M1", 2 * j, W1, m, BLACK)), j


@pytest.mark.parametrize("name", ["M1", "D1"])
def test_bilinear_one_channel(device, monkeypatch, name):
    """affine_bilinear_kernel<1>: channel 0 of the frames as a one-channel image."""
    from imagetransformations_amd import ops
    _set_knobs(monkeypatch, {})
    m = tuple(MATS[name][0])
    for i in (0, 7):
        t = dev(_variants(name, 0)[i], device)
        assert bilinear_route(t, m, W0) == ("global1", False)
        got = host(ops.affine(t, m, W0, ops.BILINEAR, (9,), precise=True))
        assert np.array_equal(got, _ref("bilinear", name, i, W0, m, (9,), 0)), i


FP32_CASES = [("wq", False, "M1", 5, W0, {}), ("wq", False, "D2", 5, W0, {}), ("mf13_dma", False, "M1", 5, W1, {}),
              ("mf13", True, "M1", 5, W1, {"NO_DMA": 1}), ("lds_interior", True, "M1", 1, W0, {}),
              ("lds49", False, "M3", 3, W0, {}), ("global3", False, "M1", 3, W0, {"NO_LDS": 1})]


@pytest.mark.parametrize("route,lists,name,n,size,knobs", FP32_CASES, ids=[f"{c[0]}-{c[2]}" for c in FP32_CASES])
def test_bilinear_fp32_mode_within_tolerance(device, monkeypatch, route, lists, name, n, size, knobs):
    """precise=False: every byte is the truncation of ref - tol or of ref + tol, tol = 1e-5 max(|ref|, 1).
    No cap on the share of differing bytes: on this corpus the reference puts thousands of bytes inside
    tol of an integer; being one of the two admissible bytes is the test."""
    from imagetransformations_amd import ops
    _set_knobs(monkeypatch, knobs)
    m = tuple(MATS[name][0])
    t = dev(_variants(name)[list(PICK[n])], device)
    assert bilinear_route(t, m, size) == (route, lists)
    got = host(ops.affine(t, m, size, ops.BILINEAR, BLACK, precise=False))
    for j, i in enumerate(PICK[n]):
        ref = np.asarray(_ref_float(name, i, size, m, BLACK)[0], np.float64)
        tol = 1e-5 * np.maximum(np.abs(ref), 1.0)
        good = (got[j] == _q(ref - tol)) | (got[j] == _q(ref + tol))
        assert good.all(), (name, i, int((~good).sum()))


@pytest.mark.parametrize("precise", [True, False])
@pytest.mark.parametrize("name,n,knobs,route", [("M1", 1, {}, ("lds_interior", True)), ("M2", 1, {}, ("lds_interior", True)),
                                                ("D2", 1, {}, ("lds_interior", True)), ("D1", 1, {}, ("lds49", False)),
                                                ("M3", 3, {}, ("lds49", False)),
                                                ("M1", 3, {"NO_LDS": 1}, ("global3", False))])
def test_bilinear_f32_side_output(device, monkeypatch, name, n, knobs, route, precise):
    """return_f32: the fp32 value is within tol of the oracle's float value on every inside pixel, and the
    bytes beside it are Pillow's (precise) or admissible (fp32 mode)."""
    from imagetransformations_amd import ops
    _set_knobs(monkeypatch, knobs)
    m = tuple(MATS[name][0])
    t = dev(_variants(name)[list(PICK[n])], device)
    assert bilinear_route(t, m, W0, return_f32=True) == route
    out, f32 = ops.affine(t, m, W0, ops.BILINEAR, BLACK, precise=precise, return_f32=True)
    out, f32 = host(out), host(f32).astype(np.float64)
    for j, i in enumerate(PICK[n]):
        ref, ok = _ref_float(name, i, W0, m, BLACK)
        tol = 1e-5 * np.maximum(np.abs(ref), 1.0)
        err = np.abs(f32[j] - ref)[ok]
        assert (err <= tol[ok]).all(), (name, i, float(err.max()))
        if precise:
            assert np.array_equal(out[j], _ref("bilinear", name, i, W0, m, BLACK)), (name, i)
        else:
            assert ((out[j] == _q(ref - tol)) | (out[j] == _q(ref + tol))).all(), (name, i)


# ------------------------------------------------------------------ bicubic
WHITE = (255, 255, 255)
BICUBIC_CASES = [("B1", "B1", {}, "shear_unit_step+edges"), ("B2", "B2", {}, "shear_unit_step+edges"), ("B3", "B3", {}, "shear_rows"),
                 ("CLIP", "B1", {}, "shear_unit_step+edges"), ("CLIP", "B2", {}, "shear_unit_step+edges"), ("CLIP", "B3", {}, "shear_rows"),
                 ("B1", "B1", {"NO_SHEAR_FAST": 1}, "general"), ("B3", "B3", {"NO_SHEAR_FAST": 1}, "general"),
                 ("CLIP", "B3", {"NO_SHEAR_FAST": 1}, "general"),
                 ("B1", "G", {}, "general"), ("CLIP", "G", {}, "general")]


@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("name,mat,knobs,route", BICUBIC_CASES, ids=[f"{c[0]}-{c[1]}-{c[3]}" for c in BICUBIC_CASES])
def test_bicubic_precise_equals_pillow(device, monkeypatch, name, mat, knobs, route, n):
    """shear_bicubic_kernel<true, true> + shear_edges_kernel, shear_bicubic_kernel<true, false>, the general
    kernel, and a matrix with m3 != 0 (fp64 arithmetic throughout: the control that needs no guard)."""
    from imagetransformations_amd import ops
    _set_knobs(monkeypatch, knobs)
    m, size = (C.BICUBIC_GENERAL, C.BICUBIC["B1"][1]) if mat == "G" else C.BICUBIC[mat]
    m = tuple(m)
    t = dev(_variants(name)[list(PICK[n])], device)
    assert bicubic_route(t, m) == route
    got = host(ops.affine(t, m, size, ops.BICUBIC, WHITE, precise=True))
    for j, i in enumerate(PICK[n]):
        want = _ref("bicubic", name, i, size, m, WHITE)
        assert np.array_equal(got[j], want), (name, i, int((got[j] != want).sum()))
