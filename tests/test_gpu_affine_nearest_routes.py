"""Every NEAREST route of imgxf_affine_u8 against O.affine_nearest, bit for bit: the eight affine_nearest_wq_kernel
instantiations, affine_nearest_dma_kernel<64, 13> and <32, 11>, affine_nearest_lds_kernel<49 | 65 | 97> and the global
kernel for one, three and four channels.  Each case first asserts the kernel the dispatcher takes for it (`nearest_route`,
which test_affine_route_host.py holds against the host code, and the table of nearest_route_corpus.py), so a geometry
that silently moves to another kernel fails here instead of leaving a kernel untested.

The corpus (nearest_route_corpus.py) holds, beside rotations, matrices of multiples of 2^-16 whose coordinates fall on
pixel boundaries and into (-1, 0) along the left and top edges (`>> 16`, not a truncating division; the low corner of the
staged box), shifts that leave one source row or column or nothing visible, and boxes on the last 16-byte chunk of a
row.  The output sizes 100 x 70 and 37 x 29 end in partial tiles: row tails of 4 and 1 pixels, stores by dwords and by
bytes."""
import functools

import numpy as np
import pytest
import torch

import nearest_route_corpus as N
from affine_route import nearest_refused, nearest_route
from oracle import imgxf_oracle as O
from test_gpu_parity import host

pytestmark = pytest.mark.gpu


def dev(a, device):
    return torch.from_numpy(np.array(a)).to(device)          # a copy: the corpus arrays are read-only


def _fill(c):
    return (N.FILL + (6,))[:c]


@functools.lru_cache(maxsize=None)
def _ref(name, size, i, c=3):
    """O.affine_nearest of corpus frame i, computed once."""
    out = O.affine_nearest(N.frames(c)[i % 4], N.SIZES[size], list(N.matrix(name, size)), fill=_fill(c))
    out.setflags(write=False)
    return out


def _set_knobs(monkeypatch, knobs):
    for k in ("FPB", "NO_DMA", "NO_LDS", "NO_TALL", "NO_SHEAR_FAST"):
        monkeypatch.delenv("IMGXF_AFFINE_" + k, raising=False)
    for k, v in knobs.items():
        monkeypatch.setenv("IMGXF_AFFINE_" + k, str(v))


def _offset_view(a, byte_offset, device):
    """The batch `a` on the device in storage that starts `byte_offset` bytes after a 16-byte aligned address."""
    buf = torch.zeros(a.size + 64, dtype=torch.uint8, device=device)
    assert buf.data_ptr() % 16 == 0
    v = buf[byte_offset:byte_offset + a.size].view(a.shape)
    v.copy_(torch.from_numpy(np.ascontiguousarray(a)))
    return v


def _run(device, name, size, t, route, frame_ids, c=3):
    from imagetransformations_amd import ops
    m = N.matrix(name, size)
    assert nearest_route(t, m, N.SIZES[size]) == route, (name, size)
    got = host(ops.affine(t, m, N.SIZES[size], ops.NEAREST, _fill(c)))
    got = got.reshape((len(frame_ids),) + _ref(name, size, 0, c).shape)          # a [H, W, C] or [H, W] input gives one frame
    for j, i in enumerate(frame_ids):
        want = _ref(name, size, i, c)
        assert np.array_equal(got[j], want), (name, size, route, j, f"{int((got[j] != want).any(axis=-1).sum())} pixels differ")


def _knob_id(knobs, offset):
    return "-".join([f"{k}{v}" for k, v in knobs.items()] + ([f"off{offset}"] if offset else [])) or "default"


# ------------------------------------------------------------------------------------------------- every matrix x every size
@pytest.mark.parametrize("size", list(N.SIZES))
@pytest.mark.parametrize("name", list(N.MATS))
def test_default_route_equals_oracle(device, monkeypatch, name, size):
    """Two dense frames (position, noise), no knob: the wq instantiations at the 16-byte-multiple widths, the dma / lds /
    global kernels with partial last tiles at the others."""
    _set_knobs(monkeypatch, {})
    _run(device, name, size, dev(N.batch(2), device), N.default_route(name, size), (0, 1))


# ------------------------------------------------------------------------------------------------- knobs and source offsets
VARIANTS = [({"NO_TALL": 1}, 0), ({"NO_DMA": 1}, 0), ({"NO_LDS": 1}, 0), ({}, 1), ({}, 4), ({}, 16)]
VARIANT_NAMES = ("r22.5x1", "r45x1", "r45x1.2", "r30x1.5", "dyadic1", "dyadic1.5", "first-column", "first-row", "last-column", "nothing-right")


@pytest.mark.parametrize("knobs,offset", VARIANTS, ids=[_knob_id(*v) for v in VARIANTS])
@pytest.mark.parametrize("size", ["96x80", "100x70", "37x29"])
@pytest.mark.parametrize("name", VARIANT_NAMES)
def test_knobs_and_source_offsets(device, monkeypatch, name, size, knobs, offset):
    """NO_TALL turns dma64 into dma32, NO_DMA or a source 4 bytes off a 16-byte address gives the dword-staged lds kernels,
    NO_LDS or a source 1 byte off gives the global kernel, 16 bytes off changes nothing."""
    _set_knobs(monkeypatch, knobs)
    a = N.batch(2)
    t = _offset_view(a, offset, device) if offset else dev(a, device)
    assert t.data_ptr() % 16 == offset % 16
    _run(device, name, size, t, N.expected_route(name, size, knobs, offset), (0, 1))


# ------------------------------------------------------------------------------------------------- layouts
WQ_NAMES = [name for name in N.MATS if isinstance(N.MATS[name][1], tuple)]


@pytest.mark.parametrize("fpb", [2, 3])
@pytest.mark.parametrize("name", WQ_NAMES)
def test_wq_frame_loop(device, monkeypatch, name, fpb):
    """Five frames at 2 and 3 per workgroup: the double-buffered boxes and slots of every wq instantiation, with a ragged
    last group."""
    _set_knobs(monkeypatch, {"FPB": fpb})
    _run(device, name, "96x80", dev(N.batch(5), device), N.MATS[name][1], range(5))


@pytest.mark.parametrize("size", ["80x72", "37x29"])
@pytest.mark.parametrize("name", ["r22.5x1", "r45x1", "r45x1.2", "r30x1.5", "r20x2.9", "dyadic1", "first-column"])
def test_single_frames_and_every_other_frame(device, monkeypatch, name, size):
    """A [H, W, 3] tensor, and big[::2] of a batch of six (a frame stride of two frames)."""
    _set_knobs(monkeypatch, {})
    route = N.default_route(name, size)
    for i in (0, 1):
        _run(device, name, size, dev(N.frames()[i], device), route, (i,))
    big = dev(N.batch(6), device)
    _run(device, name, size, big[::2], route, (0, 2, 4))


@pytest.mark.parametrize("aligned", [False, True], ids=["odd", "aligned16"])
@pytest.mark.parametrize("size", ["96x80", "37x29"])
@pytest.mark.parametrize("name", ["r22.5x1", "r45x1", "r45x1.2", "r30x1.5", "r20x2.9", "dyadic1", "first-column", "nothing-right"])
def test_guarded_destinations(device, monkeypatch, name, size, aligned):
    """A destination with padded rows and frames inside a canary-filled allocation: at an odd lead with odd pads every
    tile leaves by bytes through the dma / lds / global kernels; with lead and pads multiples of 16 the wq kernel's whole
    lines and the staged 96-byte segments write rows that are not packed.  The pads stay untouched."""
    from imagetransformations_amd import _ffi as F
    from test_gpu_canary import Guarded
    _set_knobs(monkeypatch, {})
    ow, oh = N.SIZES[size]
    m = N.matrix(name, size)
    t = dev(N.batch(3), device)
    g = Guarded(device, 3, oh, ow, 3, *((-(ow * 3) % 16 + 16, 32, 256) if aligned else (3, 5, 257)))
    dst16 = (g.view.data | g.view.row_stride | g.view.frame_stride) % 16 == 0
    assert dst16 == aligned
    route = N.expected_route(name, size, dst16=dst16)
    assert nearest_route(t, m, (ow, oh), dst=g.view) == route
    F.call("imgxf_affine_u8", F.vp(F.view_of(t)), F.vp(g.view), F.f64_array(list(m)), F.FILTER_NEAREST, F.u8_array(list(N.FILL) + [0]), 1,
           None, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    g.check(np.stack([_ref(name, size, i) for i in range(3)]), f"nearest {name} {size} {route}")


@pytest.mark.parametrize("c", [1, 4])
@pytest.mark.parametrize("size", ["96x80", "37x29"])
@pytest.mark.parametrize("name", ["r22.5x1", "dyadic1", "dyadic2.25", "first-column", "first-row", "last-column", "nothing-above"])
def test_one_and_four_channels(device, monkeypatch, name, size, c):
    """affine_kernel<1, NEAREST> and <4, NEAREST>: a batch, and for one channel a [H, W] plane."""
    _set_knobs(monkeypatch, {})
    a = N.batch(2, c)
    _run(device, name, size, dev(a, device), "global", (0, 1), c)
    if c == 1:
        _run(device, name, size, dev(a[1, ..., 0], device), "global", (1,), c)


# ------------------------------------------------------------------------------------------------- refused warps
@pytest.mark.parametrize("m,size", [((1092.5, 0.3, -546.0, 0.01, 0.9, 0.0), (64, 64)),       # the wrapped 16.16 coordinates land inside the source
                                    ((0.9, 0.3, 70000.0, 0.01, 0.9, 0.0), (96, 80)),
                                    ((40000.0, 0.5, -20000.0, 0.0, 1.0, 0.0), (1, 1))],      # check_fixed holds, m0 fits no 16.16 int
                         ids=["wraps-inside", "m2-70000", "m0-40000"])
def test_warps_outside_fixed_point_are_refused(device, m, size):
    """Pillow walks these in doubles; the 16.16 kernels would return other pixels, so the call raises and the C entry
    point returns IMGXF_ERR_UNSUPPORTED whatever the kernel it would have taken."""
    from imagetransformations_amd import _ffi as F, ops
    assert nearest_refused(m, size)
    t = dev(N.batch(2), device)
    with pytest.raises(ValueError, match="16.16 fixed point"):
        ops.affine(t, m, size, ops.NEAREST, N.FILL)
    out = torch.full((2, size[1], size[0], 3), 0xA5, dtype=torch.uint8, device=device)
    rc = F.lib.imgxf_affine_u8(F.vp(F.view_of(t)), F.vp(F.view_of(out)), F.f64_array(list(m)), F.FILTER_NEAREST, F.u8_array(list(N.FILL) + [0]),
                               1, None, torch.cuda.current_stream().cuda_stream)
    assert rc == F.ERR_UNSUPPORTED
    assert bool((out == 0xA5).all())
    ops.affine(t, m, size, ops.BILINEAR, N.FILL)             # the fp64 filters have no such limit
