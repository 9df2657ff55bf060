"""Which kernel imgxf_affine_u8 launches for a NEAREST, BILINEAR or BICUBIC geometry: a restatement of the box formulas and
alignment tests of plan_affine (imagetransformations_amd/csrc/affine_route.h) with the knobs now in the environment, for
tests that pin a geometry to a kernel (test_gpu_affine_near_integer.py, test_gpu_affine_nearest_routes.py).  test_affine_route_host.py holds it against the
host code itself, without a device; a change to the limits in csrc changes these functions with it."""
import math
import os


def _box(m, tw, th, extra=4):
    return (math.ceil(abs(m[0]) * (tw - 1) + abs(m[1]) * (th - 1)) + extra,
            math.ceil(abs(m[3]) * (tw - 1) + abs(m[4]) * (th - 1)) + extra)


def _llround(v):
    return int(math.copysign(math.floor(abs(v) + 0.5), v))


def _fix16(v):
    return int(math.floor(v * 65536.0 + 0.5))


def _box_fx(a, b, tw, th, extra=3):
    return math.ceil((abs(a) * (tw - 1) + abs(b) * (th - 1)) / 65536.0) + extra


def nearest_refused(m, out_size):
    """plan_affine's IMGXF_ERR_UNSUPPORTED for NEAREST: libImaging's check_fixed fails at a corner of the output, or a
    coefficient of the 16.16 matrix fits no int."""
    ow, oh = out_size
    at = lambda x, y: abs(x * m[0] + y * m[1] + m[2]) < 32768.0 and abs(x * m[3] + y * m[4] + m[5]) < 32768.0
    coeffs = (m[0], m[1], m[2] + m[0] * 0.5 + m[1] * 0.5, m[3], m[4], m[5] + m[3] * 0.5 + m[4] * 0.5)
    return not (at(0, 0) and at(ow, oh) and at(0, oh) and at(ow, 0)) or not all(abs(c * 65536.0 + 0.5) < 2147483648.0 for c in coeffs)


def nearest_route(t, m, out_size, dst=None):
    """The kernel that run_affine takes for NEAREST (m1 or m3 non-zero, not refused) on source tensor `t` with the knobs
    now in the environment: ("wq", kw), "dma64", "dma32", "lds49", "lds65", "lds97" or "global".  The destination is the
    view `dst`, or the fresh contiguous tensor ops.affine makes (16-byte aligned base, rows of 3 ow bytes)."""
    from imagetransformations_amd import _ffi as F
    s = F.view_of(t)
    ow, oh = out_size
    env = os.environ
    assert not nearest_refused(m, out_size) and s.n <= 65535
    if s.c != 3 or "IMGXF_AFFINE_NO_LDS" in env or (s.data | s.row_stride | s.frame_stride) & 3:
        return "global"
    fx = [_fix16(m[0]), _fix16(m[1]), _fix16(m[2] + m[0] * 0.5 + m[1] * 0.5),
          _fix16(m[3]), _fix16(m[4]), _fix16(m[5] + m[3] * 0.5 + m[4] * 0.5)]
    corners = [(X, Y) for Y in (0, oh + 32) for X in (0, ow + 32)]
    nowrap = all(abs(fx[2] + fx[1] * Y + fx[0] * X) <= 2.0e9 and abs(fx[5] + fx[4] * Y + fx[3] * X) <= 2.0e9 for X, Y in corners)
    bw, bh = _box_fx(fx[0], fx[1], 32, 32), _box_fx(fx[3], fx[4], 32, 32)
    if not (nowrap and bw <= 97 and bh <= 100):
        return "global"
    no_dma = "IMGXF_AFFINE_NO_DMA" in env
    src16 = (s.data | s.row_stride | s.frame_stride) % 16 == 0 and (s.w * 3) % 16 == 0 and s.w * 3 >= 16
    d = (0, ow * 3, oh * ow * 3) if dst is None else (dst.data, dst.row_stride, dst.frame_stride)
    dst16 = (d[0] | d[1] | d[2]) % 16 == 0 and (ow * 3) % 16 == 0
    bwq, bhq = _box_fx(fx[0], fx[1], 32, 16), _box_fx(fx[3], fx[4], 32, 16)
    kw = (bhq * ((bwq * 3 + 30) // 16) + 63) // 64
    if src16 and dst16 and not no_dma and kw <= 8:
        return "wq", kw
    if bw <= 49 and bh <= 52 and not no_dma and src16:
        bw64, bh64 = _box_fx(fx[0], fx[1], 32, 64), _box_fx(fx[3], fx[4], 32, 64)
        return "dma64" if bw64 <= 64 and bh64 <= 80 and "IMGXF_AFFINE_NO_TALL" not in env else "dma32"
    return "lds49" if bw <= 49 else "lds65" if bw <= 65 else "lds97"


def bilinear_route(t, m, out_size, return_f32=False):
    """(kernel, uses the list kernel too) that run_affine takes for BILINEAR on source tensor `t` with
    the knobs now in the environment; the destination is the fresh contiguous tensor ops.affine makes."""
    from imagetransformations_amd import _ffi as F
    s = F.view_of(t)
    ow, oh = out_size
    env = os.environ
    align = lambda *v: all(int(x) % 16 == 0 for x in v)
    if s.c == 1:
        return "global1", False
    if "IMGXF_AFFINE_NO_LDS" in env or (s.data | s.row_stride | s.frame_stride) & 3:
        return "global3", False
    (bw, bh), (bwt, bht), (bwq, bhq) = _box(m, 32, 32), _box(m, 32, 64), _box(m, 32, 16)
    assert bw <= 97 and bh <= 100
    ntx = (ow + 31) // 32
    if "IMGXF_AFFINE_NO_TALL" not in env and bwt <= 49 and bht <= 64 and bw <= 49:
        no_dma = "IMGXF_AFFINE_NO_DMA" in env
        mf = not return_f32 and int(env.get("IMGXF_AFFINE_FPB", 16)) >= 2 and s.n >= 2
        src16 = align(s.data, s.row_stride, s.frame_stride) and s.w * 3 >= 16
        nch, nchq = (bwt * 3 + 30) // 16, (bwq * 3 + 30) // 16
        if mf and not no_dma and src16 and align(ow * 3, oh * ow * 3) and bwq <= 28 and bhq * nchq <= 192 and bhq * 7 <= 192:
            return "wq", False
        if mf and not no_dma and src16 and bht <= 52 and bwt <= 52 and 52 * nch <= 768:
            return "mf13_dma", False
        # tiles that are not interior go to the list kernel (the host's integers, 2^-40 units)
        q = [_llround(v * 2.0 ** 40) for v in m]
        x00 = math.floor(((m[0] * 0.5 + m[1] * 0.5) + m[2] - 0.5) * 2.0 ** 40)
        y00 = math.floor(((m[3] * 0.5 + m[4] * 0.5) + m[5] - 0.5) * 2.0 ** 40)
        ntyt, listed = (oh + 63) // 64, 0
        for ty in range(ntyt):
            for tx in range(ntx):
                xt, yt = x00 + tx * 32 * q[0] + ty * 64 * q[1], y00 + tx * 32 * q[3] + ty * 64 * q[4]
                xs, ys = (0, 31 * q[0], 63 * q[1], 31 * q[0] + 63 * q[1]), (0, 31 * q[3], 63 * q[4], 31 * q[3] + 63 * q[4])
                xlo, xhi, ylo, yhi = (xt + min(xs)) >> 40, ((xt + max(xs)) >> 40) + 1, (yt + min(ys)) >> 40, ((yt + max(ys)) >> 40) + 1
                clean = (xlo >= 0 and ylo >= 0 and xhi <= s.w - 1 and yhi <= s.h - 1 and tx * 32 + 32 <= ow and ty * 64 + 64 <= oh
                         and not (xhi == s.w - 1 and yhi == s.h - 1))
                listed += not clean
        assert listed <= 896
        if listed < ntx * ntyt:
            return ("mf13" if bht <= 52 else "mf16") if mf else "lds_interior", listed > 0
        return "lds_list_only", True
    return ("lds49" if bw <= 49 else "lds65" if bw <= 65 else "lds97"), False


def bicubic_route(t, m):
    """run_affine's choice for BICUBIC, three channels, no fp32 side output."""
    honly = m[3] == 0.0 and m[4] == 1.0 and m[5] == math.floor(m[5]) and abs(m[5]) < 1.0e9
    if honly and "IMGXF_AFFINE_NO_SHEAR_FAST" not in os.environ and t.shape[-2] >= 4:
        return "shear_unit_step+edges" if m[0] == 1.0 else "shear_rows"
    return "general"
