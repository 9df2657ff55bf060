"""What a Sobel call launches, asked of the library itself: imgxf_sobel_plan_host (plan_sobel in csrc/sobel_march.inc, the
function the entry points launch from).  Needs the built library, no device.  Not a restatement of the rule: the tests
that choose geometries from it (test_gpu_sobel.py) and the test of the rule's values (test_sobel_plan_host.py) share it."""
import ctypes
from collections import namedtuple

Plan = namedtuple("Plan", "march nstrips spb rpw nchunks nchunks0 grid threads lds launches")


def plan_views(src, dst):
    """Plan of the entry point that takes `src` (c == 1: imgxf_sobel_u8, c == 3: imgxf_rgb_sobel_u8) and `dst`, two
    _ffi.View.  Reads IMGXF_NO_MARCH as the library has it cached."""
    from imagetransformations_amd import _ffi as F
    out = (ctypes.c_int * F.SOBEL_PLAN_INTS)(*([-1] * F.SOBEL_PLAN_INTS))
    rc = F.lib.imgxf_sobel_plan_host(ctypes.byref(src), ctypes.byref(dst), out)
    assert rc == F.OK, rc
    o = list(out)
    return Plan(bool(o[0]), o[1], o[2], o[3], o[4], o[5], tuple(o[6:9]), o[9], o[10], o[11])


def plan(n, h, w, cin=1, src_base=4096, dst_base=1 << 20, src_rs=None, src_fs=None, dst_rs=None, dst_fs=None):
    """Plan for [n,h,w,cin] -> [n,h,w,1] views that are dense unless a stride is given; the addresses are only looked at."""
    from imagetransformations_amd import _ffi as F
    src_rs = w * cin if src_rs is None else src_rs
    dst_rs = w if dst_rs is None else dst_rs
    src = F.View(src_base, n, h, w, cin, src_rs, src_rs * h if src_fs is None else src_fs)
    dst = F.View(dst_base, n, h, w, 1, dst_rs, dst_rs * h if dst_fs is None else dst_fs)
    return plan_views(src, dst)


def chunk_rows(p, h):
    """Rows of every chunk of a marching plan, in order."""
    return [min(p.rpw, h - y) for y in range(0, h, p.rpw)]
