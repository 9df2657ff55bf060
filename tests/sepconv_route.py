"""Which kernel family and radius the separable-filter dispatchers launch: a restatement of the host code in
imagetransformations_amd/csrc, at the default knobs, for tests that must know it without a device
(test_sepconv_route.py) or that pin a geometry to a kernel (test_gpu_sepconv_channels.py, test_gpu_sepconv_borders.py).
test_sepconv_route.py holds it to the planner (csrc/sepconv_route.h) through tools/sepconv_launch_trace.hip, so a change
to the limits in csrc changes this function with it.  conv2d_separable() is no restatement: it asks the library's host
function whether filter2D hands a kernel to these dispatchers at all."""
REFLECT_101, REFLECT = 0, 1                     # include/imgxf.h: IMGXF_BORDER_REFLECT_101, IMGXF_BORDER_REFLECT


def _march_eligible(c, R, h, w, aligned, border):
    """sepconv_route.h: march_eligible"""
    rb = w * c
    return (border == REFLECT_101 and (R + 1) * c <= 16 and w >= R + 1 and h >= R + 1
            and rb % 16 == 0 and rb > 1024 and aligned)


def _march4_eligible(c, R, h, w, aligned, border):
    """sepconv_route.h: march4_eligible"""
    rb = w * c
    return (border == REFLECT_101 and 1 <= R <= 15 and w >= R + 1 and h >= R + 1
            and rb % 16 == 0 and rb >= 256 + 32 * ((R * c + 15) // 16) and aligned)


def _mfma_eligible(c, R, h, w, aligned, border, taps_fit_mfma):
    """sepconv_route.h: mfma_views_eligible, without the tap tests of mfma_eligible (float) and fx_mfma_eligible (fixed),
    which the caller states as taps_fit_mfma; frames of 4 GiB and more are not restated."""
    rb = w * c
    return (c == 3 and border == REFLECT_101 and taps_fit_mfma and 2 <= R <= 15 and w >= 17 and h >= 32
            and rb % 16 == 0 and rb >= 256 and aligned)


def sepconv_route(c, fixed, R, h, w, *, aligned=True, border=REFLECT_101, sym=True, f32=False, taps_fit_mfma=True):
    """("tile" | "march" | "march4" | "mfma", R) for a [h][w][c] frame and a filter of radius R = max(nkx, nky) // 2.

    aligned: base addresses, row and frame strides of source, destination and fp32 output are multiples of 16.
    sym: kx is symmetric and ky == kx (every Gaussian); it selects the SYM instantiation of the marching-4 kernel and
    is a condition of the fixed-point one.  f32: an fp32 side output is asked for (float path only).
    taps_fit_mfma: the range tests of mfma_eligible / fx_mfma_eligible hold (normalised Gaussians: yes)."""
    if c == 3:                                                              # route_family; march_has, mfma_has, march4_has
        if 1 <= R <= 4 and _march_eligible(3, R, h, w, aligned, border):
            return "march", R
        if fixed:
            if R >= 5 and not f32 and _mfma_eligible(3, R, h, w, aligned, border, taps_fit_mfma):
                return "mfma", R                                            # SepconvKnobs::fx_mfma_min_r
            if not sym:
                return "tile", R
        elif R >= 6 and _mfma_eligible(3, R, h, w, aligned, border, taps_fit_mfma):
            return "mfma", R                                                # SepconvKnobs::mfma_min_r
        if 5 <= R <= 15 and _march4_eligible(3, R, h, w, aligned, border):
            return "march4", R
        return "tile", R
    march_max = {1: 5, 4: 3}[c]                                             # march_max_r
    if 1 <= R <= march_max and _march_eligible(c, R, h, w, aligned, border):
        return "march", R
    if (sym or not fixed) and march_max < R <= 15 and _march4_eligible(c, R, h, w, aligned, border):
        return "march4", R
    return "tile", R                                                        # tile_has: R = 1 ... 15


def conv2d_separable(K):
    """(separable, kx, ky) of imgxf_conv2d_separable_host for the kernel K as the library gets it (float32): whether
    imgxf_conv2d_u8 hands it to the separable dispatcher (images of 1, 3 or 4 channels, default knobs) and the float32
    taps it hands on.  Not a restatement: the library's own host function, callable without a device."""
    import ctypes

    import numpy as np
    from imagetransformations_amd import _ffi
    k = np.ascontiguousarray(K, np.float32)
    kh, kw = k.shape
    sep = ctypes.c_int(-1)
    kx, ky = np.full(kw, np.nan, np.float32), np.full(kh, np.nan, np.float32)
    fp = ctypes.POINTER(ctypes.c_float)
    rc = _ffi.lib.imgxf_conv2d_separable_host(k.ctypes.data_as(fp), kh, kw, ctypes.byref(sep), kx.ctypes.data_as(fp),
                                              ky.ctypes.data_as(fp))
    assert rc == _ffi.OK and sep.value in (0, 1), (rc, sep.value)
    return bool(sep.value), kx, ky


def required_instances():
    """Every instantiation the gray and RGBA dispatchers can launch, as (c, fixed, family, R, sym): sym is False only for
    the float marching-4 kernel's asymmetric-tap instances, the one place where it picks another kernel body."""
    need = set()
    for c, march_max in ((1, 5), (4, 3)):
        for fixed in (False, True):
            need |= {(c, fixed, "march", R, True) for R in range(1, march_max + 1)}
            need |= {(c, fixed, "march4", R, True) for R in range(march_max + 1, 16)}
            need |= {(c, fixed, "tile", R, True) for R in range(1, 16)}
        need |= {(c, False, "march4", R, False) for R in range(march_max + 1, 16)}
    return need


def instance(c, fixed, R, h, w, sym=True, **kw):
    """The element of required_instances() that a case exercises."""
    family, R = sepconv_route(c, fixed, R, h, w, sym=sym, **kw)
    return c, fixed, family, R, sym or family != "march4" or fixed
