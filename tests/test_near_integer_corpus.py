"""Conditions on the reference alone that keep test_gpu_affine_near_integer.py from being vacuous:
the stored near-integer frames (near_integer_corpus.py) really put thousands of Pillow's fp64 values
just below / just above / exactly on an integer, rounding the final value to fp32 really changes
bytes, and the oracle equals Pillow byte for byte on every frame and variant.  No device.

Measured counts: profiles/near_integer_corpus.txt."""
import numpy as np
import pytest

import near_integer_corpus as C
from oracle import imgxf_oracle as O

FILLS = [(0, 0, 0), (9, 8, 7), (255, 255, 255)]


def _float(kind, a, name):
    m, size = {**C.BILINEAR, **C.DYADIC, **C.BICUBIC}[name]
    fn = O.affine_bicubic if kind == "bicubic" else O.affine_bilinear
    v, ok = fn(a, size, m, return_float=True)
    return v, np.repeat(ok[:, :, None], 3, 2)


def test_stored_frames_are_what_the_generator_writes():
    """All are 96 x 160 x 3; the cheapest one (B2, two seconds) is regenerated.  The other tests here
    verify the properties of the stored frames themselves."""
    for name in list(C.BILINEAR) + list(C.BICUBIC):
        assert C.frame(name).shape == (C.H, C.W, 3) and C.frame(name).dtype == np.uint8
    assert np.array_equal(C.generate("B2"), C.frame("B2"))


@pytest.mark.parametrize("name", list(C.BILINEAR))
def test_bilinear_density(name):
    v, ok = _float("bilinear", C.frame(name), name)
    d = C.density(v, ok)
    print(name, d)
    assert d["below13"] >= 1500 and d["above13"] >= 1500, d
    assert d["below17"] >= 300 and d["above17"] >= 300, d


@pytest.mark.parametrize("name", list(C.BICUBIC))
def test_bicubic_density(name):
    v, ok = _float("bicubic", C.frame(name), name)
    d = C.density(v, ok)
    print(name, d)
    assert d["below13"] + d["above13"] + d["exact"] >= 0.10 * d["inside"], d
    assert d["below17"] >= 1 and d["above17"] >= 1, d


def test_tuned_supports_are_not_flat():
    """Every inside bilinear byte within 2^-13 of an integer (not on it) has a non-flat 2x2 support by
    construction of the value; what is asserted is that the tuned frames hold no large flat area that
    would exempt pixels from the hand-back: under 1 % of the 2x2 windows are flat in any channel."""
    for name in C.BILINEAR:
        a = C.frame(name).astype(np.int16)
        flat = (a[:-1, :-1] == a[:-1, 1:]) & (a[:-1, :-1] == a[1:, :-1]) & (a[:-1, :-1] == a[1:, 1:])
        assert flat.mean() < 0.01, name


@pytest.mark.parametrize("kind,name", [("bilinear", n) for n in C.BILINEAR] + [("bicubic", n) for n in C.BICUBIC])
def test_rounding_the_value_to_fp32_changes_bytes(kind, name):
    """Discriminating power, on every tuned frame and each of its 12 variants: at least 20 bytes change
    when the final fp64 value is rounded to fp32 before the floor.  (The dyadic frames are exempt by
    construction: their values are integers, which fp32 holds.)"""
    for i, a in enumerate(C.variants(C.frame(name))):
        v, ok = _float(kind, a, name)
        n = C.flipped_by_fp32(v, ok)
        assert n >= 20, (name, i, n)


@pytest.mark.parametrize("name", list(C.DYADIC))
def test_dyadic_values_are_integers_on_non_flat_supports(name):
    a = C.frame(name)
    v, ok = _float("bilinear", a, name)
    d = C.density(v, ok)
    print(name, d)
    assert d["exact"] >= 0.90 * d["inside"], d
    # no 2x2 window of the frame is flat in any channel, so none of those supports is
    b = a.astype(np.int16)
    assert (b[:, :-1] != b[:, 1:]).all() and (b[:-1] != b[1:]).all()
    assert (a % 16 == 0).all()


def test_clip_frame_overshoots_both_ways():
    a = C.clip_frame(C.H, C.W, C.SEEDS["CLIP"])
    assert set(np.unique(a)) == {0, 255}
    for name in C.BICUBIC:
        v, ok = _float("bicubic", a, name)
        v = v[ok]
        assert (v < 0).sum() >= 100 and (v > 255).sum() >= 100 and (v == 0).sum() >= 100 and (v == 255).sum() >= 100, name


def _pillow(a, size, m, resample, fill):
    from PIL import Image
    return np.asarray(Image.fromarray(a).transform(size, Image.AFFINE, tuple(m), resample, fillcolor=fill))


@pytest.mark.parametrize("name", list(C.BILINEAR) + list(C.DYADIC))
def test_oracle_equals_pillow_bilinear(name):
    Image = pytest.importorskip("PIL.Image")
    m, size = {**C.BILINEAR, **C.DYADIC}[name]
    sizes = [size, (150, 96)] if name in ("M1", "D1") else [size]
    for i, a in enumerate(C.variants(C.frame(name))):
        for sz in sizes:
            for fill in FILLS:
                assert np.array_equal(O.affine_bilinear(a, sz, m, fill=fill), _pillow(a, sz, m, Image.BILINEAR, fill)), (name, i, sz, fill)


@pytest.mark.parametrize("name", list(C.BICUBIC) + ["CLIP"])
def test_oracle_equals_pillow_bicubic(name):
    Image = pytest.importorskip("PIL.Image")
    cases = [C.BICUBIC[name]] if name != "CLIP" else list(C.BICUBIC.values())
    cases = cases + [(C.BICUBIC_GENERAL, cases[0][1])]
    for i, a in enumerate(C.variants(C.frame(name))):
        for m, size in cases:
            for fill in FILLS:
                assert np.array_equal(O.affine_bicubic(a, size, m, fill=fill), _pillow(a, size, m, Image.BICUBIC, fill)), (name, i, m, fill)
