"""The affine dispatcher's choice, read off the host code without a device: tools/affine_launch_trace.hip (affine.hip
with the launch macro turned into a recorder) runs a grid of geometries, and the instantiations it records must be the
routes that affine_route.py states for the GPU tests.  The grid holds every geometry of test_gpu_affine_near_integer.py
and of nearest_route_corpus.py (test_gpu_affine_nearest_routes.py), and every route name must be reached, so neither side
can drift and no route can drop out unnoticed.  NEAREST warps that libImaging takes out of 16.16 fixed point must come
back IMGXF_ERR_UNSUPPORTED without a launch."""
import itertools
import os
import re
import shutil
import subprocess
from unittest import mock

import pytest

import near_integer_corpus as C
import nearest_route_corpus as N
import test_gpu_affine_near_integer as G
from affine_route import bicubic_route, bilinear_route, nearest_refused, nearest_route

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or ("/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else None)
SRC_BASE, DST_BASE = 0x7F1000000000, 0x7F2000000000        # 16-byte aligned, as the device allocator's blocks are
NEAREST, BILINEAR, BICUBIC = 0, 1, 2
ERR_UNSUPPORTED = -4
# NEAREST warps that plan_affine refuses, with the output size: check_fixed fails at a corner (the first wraps back inside
# the source in 32-bit 16.16 integers), or a coefficient fits no int although check_fixed holds
REFUSED = [((1092.5, 0.3, -546.0, 0.01, 0.9, 0.0), (64, 64)), ((40000.0, 0.3, -546.0, 0.01, 0.9, 0.0), (64, 64)),
           ((0.9, 0.3, 70000.0, 0.01, 0.9, 0.0), (96, 80)), ((0.9, 700.0, 0.0, 0.01, 0.9, 0.0), (96, 80)),
           ((0.9, 0.01, 0.0, 0.3, 0.9, -32768.0), (96, 80)), ((0.9, 0.01, 0.0, -345.0, 0.9, 0.0), (96, 80)),
           ((40000.0, 0.5, -20000.0, 0.0, 1.0, 0.0), (1, 1))]


class FakeTensor:
    """What _ffi.view_of needs of a tensor: uint8 storage that is never touched."""

    def __init__(self, shape, ptr, stride=None):
        self.shape = tuple(shape)
        self._ptr = ptr
        self._stride = stride or tuple(itertools.accumulate((1,) + self.shape[:0:-1], lambda a, b: a * b))[::-1]

    def data_ptr(self):
        return self._ptr

    def stride(self):
        return self._stride

    def element_size(self):
        return 1


def _frames(n, offset=0, every_other=False, one_channel=False):
    if one_channel:
        return FakeTensor((C.H, C.W), SRC_BASE + offset)
    t = FakeTensor((n, C.H, C.W, 3), SRC_BASE + offset)
    if every_other:
        t._stride = (2 * t._stride[0],) + t._stride[1:]
    return t


def _nearest_frames(n, offset=0, c=3, every_other=False):
    if c == 1:
        return FakeTensor((N.H, N.W), SRC_BASE + offset)
    t = FakeTensor((n, N.H, N.W, c) if n > 1 else (N.H, N.W, c), SRC_BASE + offset)
    if every_other:
        t._stride = (2 * t._stride[0],) + t._stride[1:]
    return t


def _nearest_grid():
    """The corpus of the GPU test against batch sizes, knob sets, source offsets and output sizes; one and four channels;
    a frame stride of two frames; the refused warps."""
    g = []
    knob_sets = [{}, {"NO_DMA": 1}, {"NO_TALL": 1}, {"NO_LDS": 1}, {"FPB": 2}, {"FPB": 3}]
    for name, n, size, knobs, offset in itertools.product(N.MATS, (1, 2, 5), N.SIZES, knob_sets, (0, 1, 4, 16)):
        g.append((NEAREST, _nearest_frames(n, offset), N.matrix(name, size), N.SIZES[size], True, False, knobs))
    for name, c in itertools.product(("r22.5x1", "dyadic1"), (1, 4)):
        g.append((NEAREST, _nearest_frames(2, c=c), N.matrix(name, "96x80"), N.SIZES["96x80"], True, False, {}))
    g.append((NEAREST, _nearest_frames(5, every_other=True), N.matrix("r22.5x1", "96x80"), N.SIZES["96x80"], True, False, {}))
    for (m, size), n, knobs in itertools.product(REFUSED, (1, 5), ({}, {"NO_LDS": 1})):
        g.append((NEAREST, _nearest_frames(n), m, size, True, False, knobs))
    return g


def _grid():
    """(filter, source, matrix, (ow, oh), precise, f32, knobs) of every case."""
    g = _nearest_grid()
    mat = lambda name: tuple(G.MATS[name][0])
    for route, lists, name, n, size, knobs, fill, offset in G.CASES:
        g.append((BILINEAR, _frames(n, offset), mat(name), size, True, False, knobs))
    for route, lists, name, n, size, knobs in G.FP32_CASES:
        g.append((BILINEAR, _frames(n), mat(name), size, False, False, knobs))
    for name, n, knobs in [("M1", 1, {}), ("M2", 1, {}), ("D2", 1, {}), ("D1", 1, {}), ("M3", 3, {}), ("M1", 3, {"NO_LDS": 1})]:
        for precise in (True, False):                       # test_bilinear_f32_side_output
            g.append((BILINEAR, _frames(n), mat(name), G.W0, precise, True, knobs))
    g.append((BILINEAR, _frames(5, every_other=True), mat("M1"), G.W1, True, False, {}))
    for name in ("M1", "D1"):
        g.append((BILINEAR, _frames(1, one_channel=True), mat(name), G.W0, True, False, {}))
    g.append((BILINEAR, _frames(5), (0.8, 0.3, 5.0, -0.3, 0.8, 7.0), G.W0, True, False, {}))      # no interior tile: the list kernel alone
    # ... and the matrices against batch sizes, output sizes, knob sets, source offsets and the fp32 side output
    knob_sets = [{}, {"NO_DMA": 1}, {"NO_TALL": 1}, {"NO_LDS": 1}, {"FPB": 1}, {"FPB": 2}, {"FPB": 24}]
    for name, n, size, knobs, offset, f32 in itertools.product(G.MATS, (1, 2, 5, 12), (G.W0, G.W1), knob_sets, (0, 1, 4, 16), (False, True)):
        g.append((BILINEAR, _frames(n, offset), mat(name), size, True, f32, knobs))
    for (name, matname, knobs, route), n in itertools.product(G.BICUBIC_CASES, (1, 3)):
        m, size = (C.BICUBIC_GENERAL, C.BICUBIC["B1"][1]) if matname == "G" else C.BICUBIC[matname]
        g.append((BICUBIC, _frames(n), tuple(m), size, True, False, knobs))
    return g


def _knob_env(knobs):
    env = {k: v for k, v in os.environ.items() if not k.startswith("IMGXF_AFFINE_")}
    env.update({"IMGXF_AFFINE_" + k: str(v) for k, v in knobs.items()})
    return mock.patch.dict(os.environ, env, clear=True)


def _expected(case):
    filt, t, m, size, precise, f32, knobs = case
    with _knob_env(knobs):
        if filt == NEAREST:
            return "refused" if nearest_refused(m, size) else nearest_route(t, m, size)
        return bilinear_route(t, m, size, return_f32=f32) if filt == BILINEAR else bicubic_route(t, m)


def _case_line(case):
    from imagetransformations_amd import _ffi as F
    filt, t, m, (ow, oh), precise, f32, knobs = case
    s = F.view_of(t)
    spec = ",".join(k if k.startswith("NO_") else f"{k}={v}" for k, v in knobs.items()) or "-"
    fields = [filt, int(precise), int(f32), s.n, s.h, s.w, s.c, s.data, s.row_stride, s.frame_stride,
              oh, ow, DST_BASE, ow * s.c, oh * ow * s.c, *[float(v).hex() for v in m], spec]
    return " ".join(str(v) for v in fields)


BILINEAR_NAMES = [(r"affine_bilinear_wq_kernel<", "wq"), (r"affine_bilinear_mf_kernel<\w+, 56, 13, true>", "mf13_dma"),
                  (r"affine_bilinear_mf_kernel<\w+, 49, 13, false>", "mf13"), (r"affine_bilinear_mf_kernel<\w+, 49, 16, false>", "mf16"),
                  (r"affine_bilinear_lds_interior_kernel<\w+, 49, \w+, 64>", "lds_interior"),
                  (r"affine_bilinear_lds_kernel<\w+, 49,", "lds49"), (r"affine_bilinear_lds_kernel<\w+, 65,", "lds65"),
                  (r"affine_bilinear_lds_kernel<\w+, 97,", "lds97"),
                  (r"affine_bilinear_kernel<1,", "global1"), (r"affine_bilinear_kernel<3,", "global3")]
NEAREST_NAMES = [(r"affine_nearest_dma_kernel<64, 13>$", "dma64"), (r"affine_nearest_dma_kernel<32, 11>$", "dma32"),
                 (r"affine_nearest_lds_kernel<49>$", "lds49"), (r"affine_nearest_lds_kernel<65>$", "lds65"),
                 (r"affine_nearest_lds_kernel<97>$", "lds97"), (r"affine_kernel<[134], 0, PreciseArith, false>$", "global")]
LIST_KERNEL = r"affine_bilinear_lds_list_kernel<\w+, 49, \w+, 64>"


def _traced_route(filt, kernels):
    """The route name, in affine_route.py's words, of the instantiations one call launched."""
    if filt == NEAREST:
        if not kernels:
            return "refused"
        wq = re.match(r"affine_nearest_wq_kernel<(\d)>$", kernels[0])
        names = [name for pattern, name in NEAREST_NAMES if re.match(pattern, kernels[0])]
        return tuple(kernels) if len(kernels) != 1 else ("wq", int(wq.group(1))) if wq else names[0] if names else tuple(kernels)
    if filt == BICUBIC:
        if len(kernels) == 2 and re.match(r"shear_bicubic_kernel<\w+, true>", kernels[0]) and kernels[1] == "shear_edges_kernel":
            return "shear_unit_step+edges"
        if len(kernels) == 1 and re.match(r"shear_bicubic_kernel<\w+, false>", kernels[0]):
            return "shear_rows"
        if len(kernels) == 1 and re.match(r"affine_kernel<3, 2, ", kernels[0]):
            return "general"
        return tuple(kernels)
    lists = bool(kernels) and re.match(LIST_KERNEL, kernels[-1]) is not None
    first = kernels[:-1] if lists else kernels
    if not first:
        return ("lds_list_only", True) if lists else tuple(kernels)
    names = [name for pattern, name in BILINEAR_NAMES if re.match(pattern, first[0])]
    return (names[0], lists) if len(first) == 1 and len(names) == 1 else tuple(kernels)


def test_nearest_corpus_table_is_the_restatement():
    """The route table of nearest_route_corpus.py, which the GPU test asserts, against nearest_route (held against the host
    code below) for every knob set and source offset."""
    knob_sets = [{}, {"NO_DMA": 1}, {"NO_TALL": 1}, {"NO_LDS": 1}, {"FPB": 2}, {"FPB": 3}]
    for name, n, size, knobs, offset in itertools.product(N.MATS, (1, 2, 5), N.SIZES, knob_sets, (0, 1, 4, 16)):
        with _knob_env(knobs):
            got = nearest_route(_nearest_frames(n, offset), N.matrix(name, size), N.SIZES[size])
        assert got == N.expected_route(name, size, knobs, offset), (name, n, size, knobs, offset)


@pytest.fixture(scope="session")
def tracer(tmp_path_factory):
    if HIPCC is None:
        pytest.skip("hipcc not found")
    exe = tmp_path_factory.mktemp("affine_launch_trace") / "affine_launch_trace"
    cmd = [HIPCC, "--offload-arch=gfx950", "-std=c++17", "-O1", "-ffp-contract=off", "-rdynamic", f"-I{ROOT}/include",
           f"-I{ROOT}/imagetransformations_amd/csrc", f"{ROOT}/tools/affine_launch_trace.hip", "-o", str(exe), "-ldl"]
    res = subprocess.run(cmd, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    return exe


def test_traced_routes_are_the_restated_ones(tracer, tmp_path):
    grid = _grid()
    cases = tmp_path / "cases.txt"
    cases.write_text("".join(_case_line(c) + "\n" for c in grid))
    res = subprocess.run([str(tracer), "--cases", str(cases)], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    traced, kernels, rcs = [], [], []
    for line in res.stdout.splitlines():
        f = line.split("\t")
        if f[0] == "L":
            kernels.append(f[1])
        elif f[0] == "C":
            rcs.append(int(f[2][3:]))
            traced.append(kernels)
            kernels = []
    assert len(traced) == len(grid)
    reached = set()
    for case, kernels, rc in zip(grid, traced, rcs):
        filt, t, m, size, precise, f32, knobs = case
        route = _traced_route(filt, kernels)
        assert route == _expected(case), (kernels, t.shape, t.data_ptr() % 16, m, size, f32, knobs)
        assert rc == (ERR_UNSUPPORTED if route == "refused" else 0), (rc, m, size)
        if filt == NEAREST:
            reached.add(("global", len(t.shape) == 2 and 1 or t.shape[-1]) if route == "global" else route)
            continue
        if filt == BILINEAR:                                 # PRECISE and DBG are the call's
            flags = [re.search(r"<(true|false)", k) for k in kernels if not k.startswith("affine_bilinear_kernel")]
            assert all(fl.group(1) == str(precise).lower() for fl in flags), (kernels, precise)
            dbg = [k for k in kernels if re.match(r"affine_bilinear_lds_\w*kernel<", k)]
            assert all(re.match(r"\w+<\w+, \d+, " + str(f32).lower(), k) for k in dbg), (kernels, f32)
            reached |= {route[0], "also lists"} if route[1] and route[0] != "lds_list_only" else {route[0]}
        else:
            reached.add(route)
    assert reached == {"wq", "mf13_dma", "mf13", "mf16", "lds_interior", "lds_list_only", "lds49", "lds65", "lds97", "global1",
                       "global3", "also lists", "shear_unit_step+edges", "shear_rows", "general",
                       *[("wq", kw) for kw in range(1, 9)], "dma64", "dma32", "lds49", "lds65", "lds97", ("global", 1), ("global", 3),
                       ("global", 4), "refused"}
