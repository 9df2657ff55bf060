"""The two-pass resample kernels of csrc/lanczos.hip (the generic, windowed and LDS-staged horizontal passes, the generic,
one-row and 4-row vertical passes) behind ops.resize and ops.resize_crop: every named case of resample_route.py runs on
the views it describes, must report the route it is in the table for (imgxf_resample_plan_route, which the launch itself
asks), must equal Pillow's bytes as the oracle states them, and must leave every byte around its destination window alone."""
import ctypes

import numpy as np
import pytest
import torch

import resample_route as R
from oracle import imgxf_oracle as O

pytestmark = pytest.mark.gpu

GUARD = 0xA5
BY_NAME = {c.name: c for c in R.CASES}
RAMP_CASES = {"both_fast_lanczos", "both_fast_bilinear", "both_fast_bicubic", "both_fast_box", "both_fast_hamming"}


def _content(case, shape):
    """Uniform noise with a saturated block and a black band (negative lobes clip at both ends of the byte range); the
    per-filter cases take a diagonal ramp plus noise instead."""
    rng = np.random.default_rng(sum(map(ord, case.name)))
    n, h, w, c = shape
    if case.name in RAMP_CASES:
        ramp = (np.arange(h)[:, None] * 255.0 / max(1, h - 1) + np.arange(w)[None, :] * 255.0 / max(1, w - 1)) / 2
        a = ramp[None, :, :, None] + rng.integers(-24, 25, shape)
        return np.clip(a, 0, 255).astype(np.uint8)
    a = rng.integers(0, 256, shape, dtype=np.uint8)
    # both flat regions lie inside the frame: the edge rows and columns, where windows are clamped, stay noise, so a
    # misplaced or dropped edge coefficient changes bytes
    a[:, h // 4: max(h // 4 + 1, h // 2), w // 4: max(w // 4 + 1, w // 2)] = 255
    a[:, :, w * 5 // 8: max(w * 5 // 8 + 1, w * 3 // 4)] = 0
    if w >= 4 and h >= 4:
        a[:, :, 0] |= 1; a[:, :, -1] |= 1; a[:, 0] |= 1; a[:, -1] |= 1      # no zero byte on the border
    return a


def _views(case, device, fill=True):
    """(source view, its host copy, flat destination buffer, canvas, destination window) laid out as Case describes."""
    (h, w), c = case.in_hw, case.c
    nb = case.n * (2 if case.every_other else 1)
    left = case.src_pad[0]
    shape = (nb, h, left + w + case.src_pad[1], c)
    host = _content(case, shape) if fill else np.zeros(shape, np.uint8)
    big = torch.from_numpy(host).to(device)
    step = 2 if case.every_other else 1
    src, a = big[::step, :, left:left + w], host[::step, :, left:left + w]
    ch, cw = case.canvas_hw()
    nbytes = case.n * ch * cw * c
    flat = torch.full((nbytes + 32,), GUARD, dtype=torch.uint8, device=device)
    assert big.data_ptr() % 16 == 0 and flat.data_ptr() % 16 == 0
    canvas = flat[case.dst_off:case.dst_off + nbytes].view(case.n, ch, cw, c)
    oh, ow = case.out_hw
    return src, a, flat, canvas, canvas[:, case.Y0:case.Y0 + oh, case.X0:case.X0 + ow]


def _reported(case, src, dst):
    """(k-steps of the fused kernel or 0, Route) that the library reports for these views at the knobs now in force."""
    from imagetransformations_amd import _ffi as F
    from imagetransformations_amd import ops
    (h, w), (nw, nh) = case.in_hw, case.size
    plan = ops._plans.get(h, w, nh, nw, case.c, src.device.index or 0, case.resample, case.window)
    out = (ctypes.c_int * 5)()
    F.call("imgxf_resample_plan_route", plan, F.vp(F.view_of(src)), F.vp(F.view_of(dst)), out)
    return out[0], R.Route(R.H_NAMES[out[1]], out[2], R.V_NAMES[out[3]], out[4])


def _workspace_bytes(case, src, dst):
    """imgxf_resample_workspace_bytes_for these views: the intermediate the call will ask the caller for."""
    from imagetransformations_amd import _ffi as F
    from imagetransformations_amd import ops
    (h, w), (nw, nh) = case.in_hw, case.size
    plan = ops._plans.get(h, w, nh, nw, case.c, src.device.index or 0, case.resample, case.window)
    nbytes = ctypes.c_size_t()
    F.call("imgxf_resample_workspace_bytes_for", plan, F.vp(F.view_of(src)), F.vp(F.view_of(dst)), ctypes.byref(nbytes))
    return nbytes.value


def _mirror(case, src, dst):
    from imagetransformations_amd import _ffi as F
    vs, vd = F.view_of(src), F.view_of(dst)
    return case.mirror((vs.data, vs.row_stride, vs.frame_stride), (vd.data, vd.row_stride, vd.frame_stride))


def _run(case, src, dst):
    from imagetransformations_amd import ops
    if case.box is None:
        ops.resize(src, case.size, case.resample, out=dst)
    else:
        ops.resize_crop(src, case.size, case.box, case.resample, out=dst)


def _reference(case, a):
    l, t, r, b = case.box or (0, 0) + tuple(case.size)
    frames = [O.resize(f if case.c > 1 else f[:, :, 0], case.size, case.resample)[t:b, l:r] for f in a]
    return np.stack(frames).reshape(len(a), b - t, r - l, case.c)


def _check_guard(case, flat, canvas):
    ch, cw = case.canvas_hw()
    nbytes = case.n * ch * cw * case.c
    whole = flat.cpu().numpy().copy()
    inner = whole[case.dst_off:case.dst_off + nbytes].reshape(case.n, ch, cw, case.c)
    oh, ow = case.out_hw
    inner[:, case.Y0:case.Y0 + oh, case.X0:case.X0 + ow] = GUARD
    assert (whole == GUARD).all(), "bytes outside the destination window were written"


@pytest.mark.parametrize("case", R.CASES, ids=lambda c: c.name)
def test_two_pass_case(device, monkeypatch, case):
    src, a, flat, canvas, dst = _views(case, device)
    if not case.unaided:
        monkeypatch.setenv("IMGXF_RESAMPLE_NO_MFMA", "1")
    ksteps, route = _reported(case, src, dst)
    assert ksteps == 0, "the fused kernel would take this call"
    assert route == _mirror(case, src, dst) == case.route
    f = case.facts()                                        # two passes: the source rows the window touches, H-filtered
    assert _workspace_bytes(case, src, dst) == (case.n * f["rh"] * f["ww"] * case.c if f["need_h"] and f["need_v"] else 0)
    _run(case, src, dst)
    assert np.array_equal(dst.cpu().numpy(), _reference(case, a))
    _check_guard(case, flat, canvas)


def test_library_reaches_every_two_pass_kernel(device, monkeypatch):
    """The routes the library itself reports over the table: a routing change that leaves a kernel without a case fails
    here, whatever the restatement says."""
    got = set()
    for case in R.CASES:
        src, _, _, _, dst = _views(case, device, fill=False)
        if case.unaided:
            monkeypatch.delenv("IMGXF_RESAMPLE_NO_MFMA", raising=False)
        else:
            monkeypatch.setenv("IMGXF_RESAMPLE_NO_MFMA", "1")
        ksteps, route = _reported(case, src, dst)
        assert ksteps == 0, case.name
        got |= R.reached(route)
    assert got == R.COMPLETE


def test_fused_report_agrees_with_the_plan_and_the_workspace_query(device):
    """At the default knobs: a call is reported fused exactly when it needs no workspace, with the plan's k-steps, and
    then names no two-pass kernel; unaided cases never are."""
    from imagetransformations_amd import _ffi as F
    from imagetransformations_amd import ops
    fused = 0
    for case in R.CASES:
        src, _, _, _, dst = _views(case, device, fill=False)
        ksteps, route = _reported(case, src, dst)
        f = case.facts()
        assert (ksteps > 0) == (f["need_h"] and f["need_v"] and _workspace_bytes(case, src, dst) == 0), case.name
        if ksteps:
            (h, w), (nw, nh) = case.in_hw, case.size
            plan = ops._plans.get(h, w, nh, nw, case.c, src.device.index or 0, case.resample, case.window)
            k = ctypes.c_int(-1)
            F.call("imgxf_resample_plan_kernel", plan, ctypes.byref(k))
            assert not case.unaided and ksteps == k.value and route == ("none", 0, "none", 0), case.name
            fused += 1
        else:
            assert route == _mirror(case, src, dst), case.name
    assert fused >= 1


@pytest.mark.parametrize("name", ["v4_up", "window_130"])
def test_no_v4_knob_switches_inside_the_process(device, monkeypatch, name):
    """IMGXF_LANCZOS_NO_V4 set after a 4-row call has already run: the next call runs the one-row kernel, same bytes."""
    case = BY_NAME[name]
    src, a, flat, canvas, dst = _views(case, device)
    if not case.unaided:
        monkeypatch.setenv("IMGXF_RESAMPLE_NO_MFMA", "1")
    assert _reported(case, src, dst)[1].v == "v4"
    _run(case, src, dst)
    first = dst.cpu().numpy()
    assert np.array_equal(first, _reference(case, a))
    monkeypatch.setenv("IMGXF_LANCZOS_NO_V4", "1")
    ksteps, route = _reported(case, src, dst)
    assert ksteps == 0 and route == _mirror(case, src, dst)
    assert (route.v, route.vk) == ("fast", case.facts()["ksy"]) and (route.h, route.hk) == case.route[:2]
    dst.fill_(GUARD)
    _run(case, src, dst)
    assert np.array_equal(dst.cpu().numpy(), first)
    _check_guard(case, flat, canvas)
    monkeypatch.delenv("IMGXF_LANCZOS_NO_V4")
    assert _reported(case, src, dst)[1].v == "v4"


def test_route_query_checks_the_views_against_the_plan(device):
    case = BY_NAME["v4_up"]
    src, _, _, canvas, dst = _views(case, device, fill=False)
    _reported(case, src, dst)
    with pytest.raises(ValueError):
        _reported(case, src, canvas[:, :dst.shape[1] - 1, :dst.shape[2]])
