"""Writes tests/golden/near_integer/near_integer_frames.npz: the tuned base frames of
tests/near_integer_corpus.py (five bilinear, three bicubic; about a minute of CPU), and prints the
density table kept in profiles/near_integer_corpus.txt.  tests/test_near_integer_corpus.py verifies
the stored frames against the oracle and Pillow; nothing trusts this script.

    python tests/golden/make_near_integer_golden.py [--table-only]
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)]

import near_integer_corpus as C          # noqa: E402
from oracle import imgxf_oracle as O     # noqa: E402


def table():
    cols = ("inside", "exact", "below13", "above13", "below17", "above17", "below20", "above20")
    lines = ["corpus  " + "".join(f"{c:>9}" for c in cols) + "  flipped_by_fp32  share_within_2^-13"]
    for group, fn in ((C.BILINEAR, O.affine_bilinear), (C.DYADIC, O.affine_bilinear), (C.BICUBIC, O.affine_bicubic)):
        for name, (m, size) in group.items():
            v, ok = fn(C.frame(name), size, m, return_float=True)
            ok3 = np.repeat(ok[:, :, None], 3, 2)
            d = C.density(v, ok3)
            share = (d["below13"] + d["above13"] + d["exact"]) / d["inside"]
            lines.append(f"{name:<8}" + "".join(f"{d[c]:>9}" for c in cols) + f"{C.flipped_by_fp32(v, ok3):>17}{share:>20.4f}")
    return "\n".join(lines)


if __name__ == "__main__":
    if "--table-only" not in sys.argv:
        frames = {name: C.generate(name) for name in list(C.BILINEAR) + list(C.BICUBIC)}
        os.makedirs(os.path.dirname(C.GOLDEN), exist_ok=True)
        np.savez_compressed(C.GOLDEN, **frames)
    print(table())
