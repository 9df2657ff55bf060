"""CPU: the progressive writer's restatement (tests/jpeg_progressive_writer_ref.py) pinned byte for byte to what the
installed Pillow writes with `progressive=True`, over shapes × qualities × subsampling spellings × RGB / "L" and three
edge constructions that each trigger an EOB-run rule (the 0x7FFF cap, the 937-bit correction-buffer flush, dummy blocks
in the DC scans only); `jpeg.header(progressive=True)` against Pillow's segments up to SOF2."""
import io

import numpy as np
import pytest
from PIL import Image, ImageFile

import jpeg_progressive_writer_ref as P
from imagetransformations_amd import jpeg

SHAPES = [(1, 1), (1, 17), (7, 9), (8, 8), (9, 16), (17, 33), (37, 53), (64, 48), (375, 500), (500, 333)]   # (h, w)
QUALITIES = (1, 75, 100)
SUBSAMPLINGS = (-1, 0, 1, 2, "4:4:4", "4:2:2", "4:2:0")


def pil_bytes(a, **params):
    b = io.BytesIO()
    keep = ImageFile.MAXBLOCK
    ImageFile.MAXBLOCK = max(keep, 8 * a.shape[0] * a.shape[1] + 65536)   # progressive output is buffered whole
    try:
        Image.fromarray(a).save(b, "JPEG", progressive=True, **params)
    finally:
        ImageFile.MAXBLOCK = keep
    return b.getvalue()


def frame(seed, h, w, gray):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    base = 128 + 70 * np.sin(xx / 9.0 + seed) + 50 * np.cos(yy / 7.0)
    a = np.clip(base[..., None] + rng.normal(0, 12, (h, w, 3)) + np.array([10, -20, 30]), 0, 255).astype(np.uint8)
    return np.asarray(Image.fromarray(a).convert("L")) if gray else a


def coefficient_frame(h=96, w=128, seed=11):
    """Grayscale, block by block the inverse DCT of DC 0 and 63 AC values of magnitude 4..6 with random signs, + 128,
    rounded: at quality 100 / 95 every coefficient stays above 1 in the last refinement scan."""
    rng = np.random.default_rng(seed)
    u = np.arange(8)
    m = np.cos((2 * u[None, :] + 1) * u[:, None] * np.pi / 16) / 2
    m[0] /= np.sqrt(2)
    out = np.zeros((h, w))
    for by in range(h // 8):
        for bx in range(w // 8):
            c = rng.integers(4, 7, (8, 8)) * rng.choice([-1, 1], (8, 8))
            c[0, 0] = 0
            out[by * 8:by * 8 + 8, bx * 8:bx * 8 + 8] = m.T @ c @ m
    return np.clip(np.round(out + 128), 0, 255).astype(np.uint8)


@pytest.mark.parametrize("h,w", SHAPES[:8], ids=lambda v: str(v))
def test_small_grid(h, w):
    rng = np.random.default_rng(h * 1000 + w)
    for q in QUALITIES:
        for s in SUBSAMPLINGS:
            for a in (rng.integers(0, 256, (h, w, 3), dtype=np.uint8), frame(q, h, w, False)):
                assert P.encode(a, q, s) == pil_bytes(a, quality=q, subsampling=s), (h, w, q, s)
                g = np.asarray(Image.fromarray(a).convert("L"))
                assert P.encode(g, q, s) == pil_bytes(g, quality=q, subsampling=s), (h, w, q, s, "L")


@pytest.mark.parametrize("h,w", SHAPES[8:], ids=lambda v: str(v))
def test_large_shapes(h, w):
    for s, gray in ((0, False), (1, False), (2, True)):
        a = frame(h + w, h, w, gray)
        assert P.encode(a, 75, s) == pil_bytes(a, quality=75, subsampling=s), (h, w, s, gray)


@pytest.mark.parametrize("ncomp", [3, 1])
@pytest.mark.parametrize("s", SUBSAMPLINGS)
def test_header_matches_pillow(s, ncomp):
    h, w = 37, 53
    a = frame(1, h, w, ncomp == 1)
    want = pil_bytes(a, quality=60, subsampling=s)
    hdr = jpeg.header(w, h, 60, ncomp=ncomp, subsampling=s, progressive=True)
    assert hdr.endswith(want[want.index(b"\xff\xc2"):want.index(b"\xff\xc4")])
    assert want.startswith(hdr)


def test_eobrun_cap():
    a = np.full((1480, 1440), 97, np.uint8)          # 33 300 luma blocks, all AC bands empty
    stats = {}
    assert P.encode(a, 75, -1, stats) == pil_bytes(a, quality=75)
    assert stats["cap_flushes"] >= 1


@pytest.mark.parametrize("q", [100, 95])
def test_correction_buffer_flush(q):
    """At quality 100 the last refinement scans flush on the 937-bit rule; at 95 the coarser quantisers bring newly
    nonzero coefficients back (no such flush), and the frame is kept as a byte check of the dense refinement path."""
    g = coefficient_frame()
    rgb = np.repeat(g[..., None], 3, 2)
    for a, s in ((g, -1), (rgb, 0)):
        stats = {}
        assert P.encode(a, q, s, stats) == pil_bytes(a, quality=q, subsampling=s)
        assert (stats["be_flushes"] >= 1) == (q == 100), stats


@pytest.mark.parametrize("h,w", [(17, 33), (37, 53)])
@pytest.mark.parametrize("s", ["4:2:0", "4:2:2"])
def test_dummy_blocks_only_in_dc_scans(h, w, s):
    a = frame(3, h, w, False)
    hs, vs = P.R.sampling(s)
    ndc = sum(1 for _ in P.R.mcu_blocks(a, 75, hs, vs))
    nown = sum(b.shape[0] * b.shape[1] for b in P.component_blocks(a, 75, hs, vs))
    assert ndc > nown                                   # the interleaved DC scans carry dummy blocks
    assert P.encode(a, 75, s) == pil_bytes(a, quality=75, subsampling=s)


def test_encode_takes_progressive():
    import inspect
    for fn in (jpeg.encode, jpeg.encode_views, jpeg.encode_device):
        assert inspect.signature(fn).parameters["progressive"].default is False
