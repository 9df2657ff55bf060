"""Where libImaging leaves 16.16 fixed point for a NEAREST warp with m1 or m3 non-zero: the one statement of the rule for
`ops.affine` and `affine_list` (csrc/imgxf_common.h: affine_check_fixed, affine_fits_fixed)."""
from __future__ import annotations

FIXED_TEXT = ("Pillow leaves 16.16 fixed point for this NEAREST warp (libImaging's check_fixed fails at a corner of the "
              "output and its float loop runs instead); this call does not follow it there")


def check_fixed(m, ow: int, oh: int) -> bool:
    """libImaging's check_fixed at the four corners of an (ow, oh) output: where it fails, a NEAREST warp with m1 or m3
    non-zero runs libImaging's float loop instead of the 16.16 `affine_fixed`."""
    def at(x, y):
        return abs(x * m[0] + y * m[1] + m[2]) < 32768.0 and abs(x * m[3] + y * m[4] + m[5]) < 32768.0
    return at(0, 0) and at(ow, oh) and at(0, oh) and at(ow, 0)


def fits_fixed(m) -> bool:
    """Whether the six coefficients of libImaging's 16.16 matrix (the half-pixel offsets folded into m2 and m5) fit the int
    they are converted to: |c| < 32768.  check_fixed alone lets |m0| up to 65536 / ow through, and C leaves the conversion of
    such a double undefined."""
    return all(abs(c * 65536.0 + 0.5) < 2147483648.0
               for c in (m[0], m[1], m[2] + m[0] * 0.5 + m[1] * 0.5, m[3], m[4], m[5] + m[3] * 0.5 + m[4] * 0.5))


def refusal(m, ow: int, oh: int) -> str | None:
    """Why a NEAREST warp with m1 or m3 non-zero is not served, or None where it is."""
    if not check_fixed(m, ow, oh):
        return f"{FIXED_TEXT} (matrix {tuple(m)}, size {(ow, oh)})"
    if not fits_fixed(m):
        return ("a coefficient of this NEAREST warp does not fit 16.16 fixed point (magnitude 32768 or more), where "
                f"libImaging's conversion is undefined: not served (matrix {tuple(m)})")
    return None
