"""The case table of test_gpu_resample_two_pass.py, held to the restated routing rule (resample_route.py) without a device:
every case takes the route it is there for, the table reaches every two-pass instantiation, and the cases that exist for
one edge of a kernel (a column group, the span limit, a width limit, a tail, a clamp) really sit on that edge."""
import numpy as np
import pytest

import resample_route as R
from oracle import imgxf_oracle as O

SRC_BASE, DST_BASE = 0x7F1000000000, 0x7F2000000000        # 16-byte aligned, as the device allocator's blocks are
BY_NAME = {c.name: c for c in R.CASES}


def _mirror(case):
    return case.mirror(*case.layout(SRC_BASE, DST_BASE))


@pytest.mark.parametrize("case", R.CASES, ids=lambda c: c.name)
def test_case_takes_its_intended_route(case):
    assert _mirror(case) == case.route
    assert case.n * (2 if case.every_other else 1) * case.in_hw[0] * (case.in_hw[1] + sum(case.src_pad)) * case.c <= 110_000
    f = case.facts()
    if case.unaided and f["need_h"] and f["need_v"]:        # why the fused kernel cannot take it: see Case
        deep = case.in_hw[1] / case.size[0] >= 2.4
        assert deep or (case.in_hw[1] * case.c) % 4 or (case.src_pad[0] * case.c) % 4, case.name


def test_table_reaches_every_two_pass_kernel():
    got = set()
    for case in R.CASES:
        got |= R.reached(_mirror(case))
    assert got == R.COMPLETE
    assert len(R.COMPLETE) == 12 + 2


def test_restated_bounds_are_pillows():
    """bounds() and ksize() against the oracle's precompute_coeffs, which carries the coefficients too."""
    for in_size, out_size in [(64, 100), (128, 96), (128, 64), (192, 64), (6, 3), (5, 2), (40, 53), (3008, 1203), (70, 49)]:
        for resample in (R.LANCZOS, R.BILINEAR, R.BICUBIC, R.BOX, R.HAMMING):
            b, _, ks = O.lanczos_coeffs(in_size, out_size, resample)
            assert ks == R.ksize(in_size, out_size, resample)
            assert np.array_equal(b, np.array(R.bounds(in_size, out_size, resample)))


def test_edge_cases_sit_on_their_edges():
    f = {name: case.facts() for name, case in BY_NAME.items()}
    # a second column group with its own base, and lanes that stage two 16-byte chunks per row
    assert f["h_lds_two_groups"]["groups"] == 2 and 256 < f["h_lds_two_groups"]["chunks"] <= 512
    assert f["h_lds_two_groups"]["hspan"] <= R.LDS_SPAN_LIMIT < f["h_fast_span_over"]["hspan"]
    assert f["h_lds_span_8191"]["hspan"] == 8191 and f["h_fast_span_8194"]["hspan"] == 8194
    for name in ("h_fast_span_over", "h_fast_span_8194"):   # the span alone keeps them off the LDS kernel
        assert (BY_NAME[name].in_hw[1] * 3) % 16 == 0 and BY_NAME[name].src_pad == (0, 0)
    # in_w == kp runs the windowed kernels, in_w == kp - 1 cannot
    for kp in (8, 12, 16):
        at, below = BY_NAME[f"h_w{kp}_kp{kp}"], BY_NAME[f"h_w{kp - 1}_kp{kp}"]
        assert at.in_hw[1] == kp and below.in_hw[1] == kp - 1
        assert f[at.name]["kpx"] == kp and f[below.name]["kpx"] == 0
        assert 8 * (kp > 8) + 4 * (kp > 12) < f[below.name]["ksx"] <= kp
    assert f["h_generic3_19taps"]["ksx"] == 19
    # the 4-row kernel: tails, the smallest height, a last group whose base is clamped to in_h - 12
    assert {BY_NAME[n].out_hw[0] % 4 for n in ("v4_tail1", "v4_tail2", "v4_tail3")} == {1, 2, 3}
    assert BY_NAME["v4_in_h12"].in_hw[0] == 12 and BY_NAME["v_fast_in_h11"].in_hw[0] == 11
    assert f["v4_up"]["v4_clamps"] and f["v4_in_h12"]["v4_clamps"]
    assert f["v_fast_13taps"]["ksy"] == 13 and f["v_fast_21taps"]["ksy"] > 16
    assert f["v_fast_union_over_12"]["ksy"] <= 12 and f["v_fast_union_over_12"]["ku4"] == 0
    # the generic vertical kernel's triggers, one at a time: the other two conditions of the fast kernels hold
    assert (BY_NAME["v_generic_rows_30_bytes"].out_hw[1] * 3) % 16 and f["v_generic_rows_30_bytes"]["ku4"]
    assert BY_NAME["v_generic_dst_off_1"].dst_off == 1 and f["v_generic_dst_off_1"]["ku4"]
    assert f["v_generic_in_h_below_taps"]["kpy"] == 0 and (BY_NAME["v_generic_in_h_below_taps"].out_hw[1] * 3) % 16 == 0
    # rows per workgroup: heights above 32 that leave a partial last block of rows, under every horizontal kernel family
    for kind in ("lds", "fast"):
        heights = {c.in_hw[0] for c in R.CASES if c.route.h == kind and c.route.v == "none"}
        assert {33, 70} <= heights
    # the byte-wise store tail: widths that are no multiple of 4, and a destination that is not 4-byte aligned
    for kind in ("lds", "fast"):
        tails = {c.out_hw[1] % 4 for c in R.CASES if c.route.h == kind}
        assert tails == {0, 1, 2, 3}
        assert any(c.dst_off & 3 for c in R.CASES if c.route.h == kind and c.route.v == "none")
    # windows: wx > 0, wy > 0, a plan that starts below the first source row, boxes that end at the last row and column
    for name in ("window_040", "window_130", "window_040_rgba", "window_130_gray"):
        case = BY_NAME[name]
        assert case.box[0] > 0 and case.box[1] > 0 and case.box[2:] == case.size
    assert f["window_040"]["ry0"] > 0 and f["window_130"]["ry0"] > 0
    # every filter on the windowed kernels and on the generic ones; batches that are every other frame
    for generic in (False, True):
        both = [c for c in R.CASES if c.route.h != "none" and c.route.v != "none"
                and (c.route.h == c.route.v == "generic") == generic and (generic or "generic" not in c.route)]
        assert {c.resample for c in both} == {R.LANCZOS, R.BILINEAR, R.BICUBIC, R.BOX, R.HAMMING}
        assert any(c.n == 3 and c.every_other for c in both)


def test_knobs_move_the_restated_route(monkeypatch):
    case = BY_NAME["both_fast_lanczos"]
    views = case.layout(SRC_BASE, DST_BASE)
    assert case.mirror(*views) == ("lds", 8, "v4", 12)
    monkeypatch.setenv("IMGXF_LANCZOS_NO_V4", "1")
    assert case.mirror(*views) == ("lds", 8, "fast", 7)
    monkeypatch.setenv("IMGXF_LANCZOS_NO_LDS", "1")
    assert case.mirror(*views) == ("fast", 8, "fast", 7)
    monkeypatch.setenv("IMGXF_LANCZOS_SLOW", "1")
    assert case.mirror(*views) == ("generic", 3, "generic", 0)


def test_route_query_rejects_null_arguments_without_a_device():
    import ctypes
    from imagetransformations_amd import _ffi
    view = _ffi.View(16, 1, 4, 4, 3, 12, 48)
    route = (ctypes.c_int * 5)()
    assert _ffi.lib.imgxf_resample_plan_route(None, ctypes.byref(view), ctypes.byref(view), route) == _ffi.ERR_NULL
