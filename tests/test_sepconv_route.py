"""sepconv_route (a restatement of the separable-filter dispatchers, tests/sepconv_route.py) against the library's own
host code where that can be asked without a device, and the parameter grids of the GPU tests mapped through it: together
they must reach every instantiation the gray and RGBA dispatchers can launch.  No device."""
import numpy as np

from oracle import imgxf_oracle as O
from sepconv_route import REFLECT, instance, required_instances, sepconv_route
from test_driver_list_blur_host import BLUR, RADII, SIZES, _ksize, _layout


def test_rgb_float_route_agrees_with_the_list_layout():
    """driver_list.layout refuses a float blur (REFUSED_FAMILY) exactly where sepconv_family_c3_dense reports another
    family than the tile kernel for the frame."""
    from imagetransformations_amd import driver_list as dl
    entries = [(f, r) for f in range(len(SIZES)) for r in RADII]
    status = _layout(entries, BLUR)["status"].tolist()
    seen = set()
    for (f, r), st in zip(entries, status):
        h, w = SIZES[f]
        family = sepconv_route(3, False, _ksize(r) // 2, h, w)[0]
        assert (family == "tile") == (st != dl.REFUSED_FAMILY), (h, w, r, family, st)
        seen.add(family)
    assert seen == {"tile", "march", "mfma"}                  # the grid reaches both answers, for both reasons


def test_route_edges():
    assert sepconv_route(1, False, 5, 6, 1040) == ("march", 5) and sepconv_route(1, False, 5, 5, 1040)[0] == "tile"
    assert sepconv_route(1, False, 5, 6, 1024)[0] == "tile"                   # rows must exceed 1 KiB; R <= 5 has no marching-4
    assert sepconv_route(1, False, 6, 7, 288) == ("march4", 6) and sepconv_route(1, False, 6, 7, 272)[0] == "tile"
    assert sepconv_route(4, False, 3, 4, 260)[0] == "march" and sepconv_route(4, False, 4, 5, 260)[0] == "march4"
    assert sepconv_route(4, False, 13, 14, 96)[0] == "march4" and sepconv_route(4, False, 13, 14, 92)[0] == "tile"
    assert sepconv_route(4, True, 5, 20, 80)[0] == "march4" and sepconv_route(4, True, 5, 20, 80, sym=False)[0] == "tile"
    assert sepconv_route(1, True, 5, 20, 1040, sym=False)[0] == "march"       # the marching kernel takes any taps
    assert sepconv_route(3, True, 5, 40, 352)[0] == "mfma" and sepconv_route(3, False, 5, 40, 352)[0] == "march4"
    assert sepconv_route(3, True, 5, 40, 352, taps_fit_mfma=False)[0] == "march4"
    for c, w in ((1, 1040), (3, 352), (4, 264)):
        for R in range(1, 16):
            assert sepconv_route(c, False, R, 40, w)[0] != "tile"
            assert sepconv_route(c, False, R, 40, w, border=REFLECT) == ("tile", R)
            assert sepconv_route(c, False, R, 40, w, aligned=False) == ("tile", R)


def _fixed_grid_of_the_gaussian_file():
    import test_gpu_gaussian_fixed as G
    sizes = (3, 5, 7, 9, 13, 19, 31)                          # test_gaussian_cv_fixed_matches_oracle's kernel sizes
    return [(c, h, w, k // 2) for h, w, c in G.SHAPES for k in sizes if k // 2 + 1 <= min(h, w)]


def test_gpu_grids_reach_every_gray_and_rgba_instantiation():
    import test_gpu_sepconv_channels as T
    hit = set()
    for c, h, w, R in T.GRID:
        hit.add(instance(c, False, R, h, w, f32=True))                        # Gaussian float, with the fp32 output
        hit.add(instance(c, True, R, h, w))                                   # Gaussian fixed
        hit.add(instance(c, False, R, h, w, sym=False, f32=True))             # asymmetric float taps, nkx != nky
    hit |= {instance(c, True, R, h, w) for c, h, w, R in _fixed_grid_of_the_gaussian_file() if c != 3}
    missing = required_instances() - hit
    assert not missing, sorted(missing)
    # the rule behind the grid: every marching frame is the narrowest eligible row, or has a short last strip
    assert all(sepconv_route(c, False, R, R + 1, w)[0] != "tile" for c, h, w, R in T.GRID if h == 70)
    assert all(sepconv_route(c, False, R, h, w)[0] == "tile" for c, h, w, R in T.GRID if h == 33 or (h, w) in T.SMALL)


def test_gpu_side_cases_take_the_families_they_name():
    import test_gpu_sepconv_borders as B
    import test_gpu_sepconv_channels as T
    fam = {(c, sepconv_route(c, False, max(nkx, nky) // 2, h, w, sym=False)[0]) for c, h, w, nkx, nky in T.SIGNED}
    assert fam == {(c, f) for c in (1, 4) for f in ("march", "march4", "tile")}
    for c, h, w, R, family in T.FIXED_ASYM:
        assert sepconv_route(c, True, R, h, w, sym=False)[0] == family
    for c, n, w, R in T.BATCHES:
        assert sepconv_route(c, False, R, T.BATCH_H, w)[0] == ("march" if R == 2 else "march4")
    for c, (h, w) in B.ALIGNED.items():
        for R in B.RADII:
            assert sepconv_route(c, False, R, h, w, f32=True)[0] != "tile" and sepconv_route(c, True, R, h, w)[0] != "tile"
            assert sepconv_route(c, False, R, h, w, border=REFLECT)[0] == "tile"


def test_references_of_the_gpu_files():
    """The integer reference equals the oracle's fixed-point Gaussian under REFLECT_101 (frames smaller than the kernel
    included), and the two borders give different bytes on the border file's frames."""
    import test_gpu_sepconv_borders as B
    import test_gpu_sepconv_channels as T
    from conftest import synth
    for h, w in T.SMALL + [(33, 35)]:
        for c in (1, 4):
            a = synth(h + w, h, w, c)
            for k in (3, 11, 31):
                taps = O.gaussian_kernel_cv_fixed(k, k / 6)
                assert taps.sum() == 256
                assert np.array_equal(T.sepconv_fixed_ref(a, taps, taps), O.gaussian_blur_cv_fixed(a, k, k / 6))
                if B.borders_can_differ(h, w, k, k):
                    assert (T.sepconv_fixed_ref(a, taps, taps, O.reflect_index) != T.sepconv_fixed_ref(a, taps, taps)).any()
    rng = np.random.default_rng(3)
    for n in (3, 11, 31):
        k = T.positive_taps(rng, n)
        assert k.dtype == np.float32 and k.min() > 0 and abs(float(k.astype(np.float64).sum()) - 1) < 1e-6
        assert sum(T.integer_taps(rng, n)) == 256
    assert not B.borders_can_differ(1, 1, 31, 31) and not B.borders_can_differ(5, 1, 1, 9) and B.borders_can_differ(5, 1, 3, 1)
