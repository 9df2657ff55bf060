"""filter2D's hand-off to the separable kernels, decided on the host (conv2d_rank1_taps in csrc/sepconv_route.h, reached
through imgxf_conv2d_separable_host): which kernels are accepted, which are refused, and that every accepted kernel is
reproduced tap by tap, |K[j][i] - ky[j] kx[i]| <= 1e-6 |K[j][i]|, by the float32 taps handed on.  The bound is recomputed
here in NumPy float64 from the returned values; it limits what the factorisation adds to a pixel to 1e-6 sum|K p|, which
the last test measures on a frame.  No GPU.

The threshold test perturbs the taps off the pivot's row and column only: that row and that column ARE the factorisation
(kx = the row, ky = the column / pivot), so a change to them moves the taps handed on, not a tap's distance from them.
(Perturbing all taps by +-d with free signs puts some taps at 4 d from the product of their row and column entries.)"""
import numpy as np
import pytest

from conftest import synth
from oracle import imgxf_oracle as O
from sepconv_route import conv2d_separable

REL = 1e-6                      # the rule's constant
ODD = range(3, 16, 2)


def f32(k):
    """The kernel as the library gets it (ops.conv2d rounds its argument to float32)."""
    return np.asarray(k, np.float64).astype(np.float32)


def tap_deviation(K, kx, ky):
    """max over the taps of |K - ky (x) kx| / |K| in float64 (0 / 0 = 0, x / 0 = inf)."""
    K = np.asarray(K, np.float32).astype(np.float64)
    dev = np.abs(K - np.outer(ky.astype(np.float64), kx.astype(np.float64)))
    with np.errstate(divide="ignore", invalid="ignore"):
        rel = np.where(dev == 0, 0.0, dev / np.abs(K))
    return float(rel.max())


def assert_accepted(K, what=""):
    sep, kx, ky = conv2d_separable(K)
    assert sep, f"{what}: refused"
    assert kx.dtype == np.float32 and ky.dtype == np.float32 and np.isfinite(kx).all() and np.isfinite(ky).all()
    d = tap_deviation(K, kx, ky)
    assert d <= REL, f"{what}: tap deviation {d}"
    return kx, ky, d


def outer_products_of_the_gpu_test():
    """The seven kernels of test_gpu_conv2d_separable.test_asymmetric_outer_products_and_generic_sepconv."""
    rng = np.random.default_rng(5)
    out = []
    for nkx, nky in [(3, 5), (7, 3), (9, 9), (11, 5), (13, 15), (15, 1), (1, 7)]:
        kx = rng.uniform(-0.2, 0.5, nkx).astype(np.float32)
        ky = rng.uniform(-0.2, 0.5, nky).astype(np.float32)
        kx /= np.float32(abs(kx.sum()) + 0.5); ky /= np.float32(abs(ky.sum()) + 0.5)
        out.append((f"outer{nky}x{nkx}", f32(np.outer(ky.astype(np.float64), kx.astype(np.float64)))))
    return out


def borders_kernels():
    from test_gpu_sepconv_borders import KERNELS
    dense = [(n, f32(k)) for n, k in KERNELS if n not in ("motion9", "box5")]
    rank1 = [(n, f32(k)) for n, k in KERNELS if n in ("motion9", "box5")]
    assert len(dense) == 4 and len(rank1) == 2
    return dense, rank1


def seeded_outer_product(seed):
    """float32 outer product of uniform(-0.2, 0.5) taps with lengths 1 ... 15 (odd) per axis.  seed % 4 == 1: 1 x n,
    2: n x 1; seed % 50 == 3: 1 x 1; seed % 3 == 0: taps decay away from a random peak down to 1e-6 of it per axis, so
    1e-12 of the pivot in the corners; seed % 5 == 0: some taps are zero; seed % 7 == 0: the pivot is negative."""
    rng = np.random.default_rng(1000 + seed)
    nkx, nky = (int(rng.choice(list(range(1, 16, 2)))) for _ in range(2))
    if seed % 4 == 1:
        nky = 1
    if seed % 4 == 2:
        nkx = 1
    if seed % 50 == 3:
        nkx = nky = 1
    v = []
    for n in (nkx, nky):
        k = rng.uniform(-0.2, 0.5, n)
        if seed % 3 == 0 and n > 1:
            peak = int(rng.integers(n))
            far = max(peak, n - 1 - peak)
            k = k * 10.0 ** (-6.0 * np.abs(np.arange(n) - peak) / far)
            k[peak] = 0.5
        if seed % 5 == 0 and n > 2:
            k[rng.random(n) < 0.3] = 0.0
        if not k.any():
            k[0] = 0.25
        v.append(k.astype(np.float32))
    kx, ky = v
    if seed % 7 == 0:
        kx = -kx if kx[np.argmax(np.abs(kx))] * ky[np.argmax(np.abs(ky))] > 0 else kx
    return f32(np.outer(ky.astype(np.float64), kx.astype(np.float64)))


def counter_example(k):
    """Every tap 0.9e-6 of the centre tap 0.499: rank 2, but each tap within 1e-6 of the LARGEST one of a rank-1 kernel."""
    K = np.full((k, k), 0.9e-6 * 0.499)
    K[k // 2, k // 2] = 0.499
    return f32(K)


def positive_rank1(k, seed):
    rng = np.random.default_rng(seed)
    kx, ky = rng.uniform(0.2, 1.0, k), rng.uniform(0.2, 1.0, k)
    return np.outer(ky / ky.sum(), kx / kx.sum())


def perturbed(k, seed, rel):
    """A positive normalised rank-1 k x k kernel whose taps off the pivot's row and column are moved by +-rel of
    themselves, signs seeded (module docstring: that row and column are the factorisation)."""
    K = positive_rank1(k, seed)
    pj, pi = np.unravel_index(np.argmax(K), K.shape)
    sign = np.random.default_rng(seed + 1).choice([-1.0, 1.0], K.shape)
    sign[pj, :] = 0.0
    sign[:, pi] = 0.0
    out = f32(K * (1.0 + rel * sign))
    assert np.unravel_index(np.argmax(out), out.shape) == (pj, pi)
    return out


JUST_INSIDE, JUST_OUTSIDE = 0.5e-6, 2e-6
# float32 rounding of the perturbed tap, of the two pivot-line entries and of ky's division: 4 x 2^-24 = 2.4e-7 at most,
# so a tap moved by 0.5e-6 deviates by 0.26e-6 ... 0.74e-6 and one moved by 2e-6 by 1.76e-6 or more
ROUNDING = 4 * 2.0 ** -24
assert JUST_INSIDE + ROUNDING < REL < JUST_OUTSIDE - ROUNDING


def accepted_kernels():
    """(name, float32 kernel) of every kernel of this file that must be accepted, but for the seeded outer products."""
    L = []
    for k in ODD:
        L += [(f"motion{k}", f32(O.motion_blur_kernel(k))), (f"box{k}", f32(O.box_kernel(k))),
              (f"2ones{k}", f32(2.0 * np.ones((k, k)) / (k * k)))]
    L += outer_products_of_the_gpu_test()
    L += [("borders:" + n, k) for n, k in borders_kernels()[1]]
    L += [("1x1", f32([[0.5]])), ("1x1 negative", f32([[-1.0]]))]
    L += [(f"inside{k}/{seed}", perturbed(k, seed, JUST_INSIDE)) for k in (5, 15) for seed in (1, 2, 3)]
    return L


def test_kernels_of_the_callers_are_accepted_and_factorised_exactly():
    for k in ODD:
        for name, K in ((f"motion{k}", O.motion_blur_kernel(k)), (f"box{k}", O.box_kernel(k)),
                        (f"2ones{k}", 2.0 * np.ones((k, k)) / (k * k))):
            assert assert_accepted(f32(K), name)[2] == 0.0, name
    for name, K in outer_products_of_the_gpu_test() + borders_kernels()[1]:
        assert_accepted(K, name)
    kx, ky, _ = assert_accepted(f32([[-1.0]]), "1x1")
    assert kx.tolist() == [-1.0] and ky.tolist() == [1.0]
    kx, ky, _ = assert_accepted(f32(O.motion_blur_kernel(5)), "motion5")
    assert kx.tolist() == [np.float32(0.2)] * 5 and ky.tolist() == [0, 0, 1, 0, 0]


def test_seeded_outer_products_are_accepted():
    worst, shapes, negative, tails, zeros = 0.0, set(), 0, 0, 0
    for seed in range(4000):
        K = seeded_outer_product(seed)
        kx, ky, d = assert_accepted(K, f"seed {seed}")
        worst = max(worst, d)
        shapes.add(K.shape)
        pivot = K.ravel()[np.argmax(np.abs(K))]
        negative += pivot < 0
        nz = np.abs(K[K != 0])
        tails += nz.min() <= 1.01e-12 * abs(pivot)
        zeros += (K == 0).any()
        assert (np.outer(ky.astype(np.float64), kx.astype(np.float64))[K == 0] == 0).all(), seed   # a zero tap: a zero product
    assert worst < 0.5 * REL, worst                 # float32 outer products sit far inside (2.3e-7 over 20 000 of them)
    assert {(1, 1), (1, 15), (15, 1), (15, 15)} <= shapes and negative > 100 and tails > 100 and zeros > 100


REFUSED = ([(f"counter-example{k}", counter_example(k)) for k in (5, 9, 15)]
           + [("eye5", f32(np.eye(5) / 5.0)), ("laplacian", f32([[0, -1, 0], [-1, 5, -1], [0, -1, 0]])),
              ("zero", np.zeros((3, 3), np.float32)), ("zero1x1", np.zeros((1, 1), np.float32)),
              ("nan", f32([[0.25, np.nan, 0.25]]))])


def test_refused_kernels():
    for name, K in REFUSED + [("borders:" + n, k) for n, k in borders_kernels()[0]]:
        sep, kx, ky = conv2d_separable(K)
        assert not sep, name
        assert np.isnan(kx).all() and np.isnan(ky).all(), name          # refused: the tap arrays are left untouched
    # a rank-1 kernel whose zero tap becomes 1e-9 of the pivot: the old rule (1e-6 of the LARGEST tap) took it
    for K in (f32(O.motion_blur_kernel(5)), f32(np.outer([0.25, 0.5, 0.25], [0.0, 0.5, 0.5]))):
        assert conv2d_separable(K)[0]
        P = np.abs(K).max()
        j, i = np.argwhere(K == 0)[0]
        K[j, i] = 1e-9 * P
        assert not conv2d_separable(K)[0]


def test_argument_checks():
    import ctypes
    from imagetransformations_amd import _ffi
    fp = ctypes.POINTER(ctypes.c_float)
    k = np.ones(16 * 16, np.float32)
    out = np.zeros(32, np.float32)
    sep = ctypes.c_int(7)
    call = _ffi.lib.imgxf_conv2d_separable_host
    kp, op = k.ctypes.data_as(fp), out.ctypes.data_as(fp)
    for kh, kw in [(0, 3), (3, 0), (2, 3), (3, 4), (17, 3), (3, 17), (-1, 1)]:
        assert call(kp, kh, kw, ctypes.byref(sep), op, op) == _ffi.ERR_ARG, (kh, kw)
    assert call(None, 3, 3, ctypes.byref(sep), op, op) == _ffi.ERR_NULL
    assert call(kp, 3, 3, None, op, op) == _ffi.ERR_NULL
    assert call(kp, 3, 3, ctypes.byref(sep), None, op) == _ffi.ERR_NULL
    assert call(kp, 3, 3, ctypes.byref(sep), op, None) == _ffi.ERR_NULL
    assert sep.value == 7
    assert call(kp, 15, 15, ctypes.byref(sep), op, op) == _ffi.OK and sep.value == 1


@pytest.mark.parametrize("k", [3, 5, 9, 15])
def test_threshold_from_both_sides(k):
    for seed in range(20):
        assert conv2d_separable(f32(positive_rank1(k, seed)))[0], (k, seed)
        inside = perturbed(k, seed, JUST_INSIDE)
        kx, ky, d = assert_accepted(inside, f"inside {k}/{seed}")
        assert JUST_INSIDE - ROUNDING <= d, (k, seed, d)                 # the perturbation is what the rule sees
        assert not conv2d_separable(perturbed(k, seed, JUST_OUTSIDE))[0], (k, seed)


def test_factorisation_moves_no_pixel_beyond_the_bound():
    """O.conv2d_f64 of the handed taps' outer product against that of K itself: at most 1e-6 sum|K p| apart per pixel
    (plus the float64 rounding of the two sums, 1e-13 of sum|K p|)."""
    a = synth(160, 40, 64)
    kernels = accepted_kernels() + [(f"seed{s}", seeded_outer_product(s)) for s in range(0, 4000, 97)]
    worst = 0.0
    for name, K in kernels:
        kx, ky, _ = assert_accepted(K, name)
        K64 = K.astype(np.float64)
        ref = O.conv2d_f64(a, K64)
        fac = O.conv2d_f64(a, np.outer(ky.astype(np.float64), kx.astype(np.float64)))
        scale = O.conv2d_f64(a, np.abs(K64))                             # sum|K p|: the pixels are not negative
        excess = np.abs(fac - ref) - (REL + 1e-13) * scale
        assert (excess <= 0).all(), (name, float(excess.max()))
        worst = max(worst, float((np.abs(fac - ref) / np.maximum(scale, 1e-300)).max()))
    assert worst > 0.2 * REL                                             # (the just-inside kernels do use the room)
