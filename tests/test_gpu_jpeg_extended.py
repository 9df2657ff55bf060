"""GPU: the extended sequential class on the device reader (`jpeg_decode.decode(..., extended=True)`:
imgxf_jpeg_layout_extended_host + imgxf_jpeg_decode_huffman_ext / _idct_ext / _color_ext) against Pillow, bit for bit:
the CPU test corpus, 4K files without restart markers (the in-segment parallel decoder), mixed batches with per-file
statuses, damaged streams, io_pipeline with IMGXF_JPEG_EXTENDED=1, and the baseline reader refusing RGB-coded files."""
import io
import os
import subprocess
import sys

import numpy as np
import pytest
from PIL import Image

import jpeg_extended_ref as R
import jpeg_sequential_writer as W
from test_jpeg_decode_oracle import photo_like
from test_jpeg_extended import SAMPLINGS, corpus, pillow_file, pillow_rgb, refusal_cases, ycck

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def large_files():
    """writer files long enough for the parallel entropy decoders: one segment (a workgroup per image), several segments of
    a few KB (a wave per segment)"""
    rng = np.random.default_rng(11)
    return [W.random_file(rng, SAMPLINGS["440"], 200, 160, noise=30, quality_scale=0.3, adobe=0),
            W.random_file(rng, SAMPLINGS["cmyk_h4"], 192, 120, noise=30, quality_scale=0.3, adobe=2),
            W.random_file(rng, SAMPLINGS["h4v2"], 256, 128, noise=30, quality_scale=0.3, restart_interval=8),
            W.random_file(rng, SAMPLINGS["cmyk_444"], 160, 128, noise=30, quality_scale=0.3, restart_interval=40)]


def test_corpus_in_one_batch_and_one_at_a_time(device):
    from imagetransformations_amd import jpeg_decode
    files = [d for _, d in corpus()] + large_files()
    frames = jpeg_decode.decode(files, device, extended=True)
    for i, (data, t) in enumerate(zip(files, frames)):
        assert np.array_equal(t.cpu().numpy(), pillow_rgb(data)), i
    for i in range(0, len(files), 9):
        assert np.array_equal(jpeg_decode.decode([files[i]], device, extended=True)[0].cpu().numpy(), pillow_rgb(files[i])), i
    assert np.array_equal(frames[3].cpu().numpy(), R.decode(files[3]))


def test_serial_entropy_decoder_gives_the_same_pixels(device, monkeypatch):
    from imagetransformations_amd import _ffi, jpeg_decode
    files = large_files()
    monkeypatch.setenv("IMGXF_JPEG_SERIAL_HUFFMAN", "1")
    _ffi.lib.imgxf_reload_knobs()
    try:
        frames = jpeg_decode.decode(files, device, extended=True)
    finally:
        monkeypatch.delenv("IMGXF_JPEG_SERIAL_HUFFMAN")
        _ffi.lib.imgxf_reload_knobs()
    for data, t in zip(files, frames):
        assert np.array_equal(t.cpu().numpy(), pillow_rgb(data))


def test_4k_cmyk_and_440_without_restart_markers(device):
    from imagetransformations_amd import jpeg_decode
    img = photo_like(12, 2160, 3840)
    cmyk = pillow_file(img, "CMYK", quality=90)
    f422 = bytearray(pillow_file(img, "RGB", quality=90, subsampling=1))
    sof = f422.index(b"\xff\xc0")
    assert f422[sof + 11] == 0x21                                 # luma h2v1; 3840 x 2160 holds as many 8 x 16 MCUs as 16 x 8
    f422[sof + 11] = 0x12                                         # -> 4:4:0, the same entropy-coded blocks
    f440 = bytes(f422)
    assert Image.open(io.BytesIO(f440)).size == (3840, 2160)
    for data in (cmyk, f440, ycck(cmyk)):
        t = jpeg_decode.decode([data], device, extended=True)[0]
        assert np.array_equal(t.cpu().numpy(), pillow_rgb(data))


def as_440(f: bytes) -> bytes:
    """a 4:2:2 file as the 4:4:0 file of the transposed size: luma sampling byte and frame size swapped, the same blocks"""
    g = bytearray(f)
    sof = g.index(b"\xff\xc0")
    assert g[sof + 11] == 0x21
    g[sof + 11] = 0x12
    g[sof + 5:sof + 7], g[sof + 7:sof + 9] = g[sof + 7:sof + 9], g[sof + 5:sof + 7]
    return bytes(g)


LANES, WAVE_PER_SEGMENT, WG256, WG1024 = range(4)


def huff_classes(files, extended):
    """csrc/jpeg_decode.hip huff_class, restated over the host layout: [(class, chunks of the first segment)] per file"""
    from imagetransformations_amd import jpeg_decode
    lay = jpeg_decode._Layout(files, False, extended)
    assert list(lay.status) == [0] * len(files)
    lay.fill()
    out = []
    for im in lay.images:
        a, b = int(lay.seg_len_h[im.seg_first]), int(lay.seg_len_h[im.seg_first + im.seg_count - 1])
        L = (a + b) // 2
        chunks256 = (L * 8 // 1024 + 255) // 256 + 1
        if L < 2048:
            cls = LANES
        elif L > 2 * 256 * 128:
            cls = WG1024
        elif im.seg_count >= 2 and L <= 16384:
            cls = WAVE_PER_SEGMENT
        else:
            cls = WG256 if im.seg_count * chunks256 * 1900 < (im.seg_count + 63) // 64 * L else LANES
        width = {WG256: 256, WG1024: 1024}.get(cls)
        nsub = (a * 8 + 1023) // 1024                                 # subsequences of PAR_BITS bits, `width` per chunk
        out.append((cls, (nsub + width - 1) // width if width else None))
    return out


def test_every_decoder_class_on_both_descriptors(device, monkeypatch):
    """Both descriptors through each of the four entropy decoders (a lane, a wave or a workgroup of 256 / 1024 per segment;
    workgroups with one chunk of subsequences and with two, where the state is carried over), asserting the class each file
    takes — a file that silently moved to another class would hide a broken kernel instance — and the pixels against
    Pillow, with the in-segment decoders and with IMGXF_JPEG_SERIAL_HUFFMAN=1."""
    from imagetransformations_amd import jpeg_decode
    P = photo_like
    baseline = [(pillow_file(P(1, 64, 64), "RGB"), LANES, None),
                (pillow_file(P(2, 48, 40), "L", restart_marker_blocks=2), LANES, None),
                (pillow_file(P(3, 256, 512), "RGB", quality=95, subsampling=0, restart_marker_rows=1), WAVE_PER_SEGMENT, None),
                (pillow_file(P(3, 256, 512), "RGB", quality=95, subsampling=2, restart_marker_rows=2), WAVE_PER_SEGMENT, None),
                (pillow_file(P(4, 160, 200), "RGB", quality=90), WG256, 1),
                (pillow_file(P(5, 200, 240), "L", quality=90), WG256, 1),
                (pillow_file(P(6, 240, 320), "RGB", quality=90, subsampling=1), WG256, 2),
                (pillow_file(P(7, 384, 512), "RGB", quality=95, subsampling=0), WG1024, 2)]
    ext = [(pillow_file(P(8, 32, 40), "CMYK", quality=80), LANES, None),                      # CMYK, RGB-coded: table period 1
           (pillow_file(P(9, 128, 512), "CMYK", quality=95, restart_marker_rows=1), WAVE_PER_SEGMENT, None),
           (pillow_file(P(10, 128, 160), "CMYK", quality=90), WG256, 1),
           (pillow_file(P(10, 160, 200), "CMYK", quality=92), WG256, 2),
           (pillow_file(P(11, 320, 384), "CMYK", quality=95), WG1024, 2),
           (pillow_file(P(12, 128, 160), "RGB", quality=90, keep_rgb=True), WG256, 1),
           (as_440(pillow_file(P(13, 40, 56), "RGB", quality=80, subsampling=1)), LANES, None),    # 4:4:0: period = 4 = blocks per MCU
           (as_440(pillow_file(P(14, 256, 512), "RGB", quality=95, subsampling=1, restart_marker_rows=2)), WAVE_PER_SEGMENT, None),
           (as_440(pillow_file(P(15, 160, 200), "RGB", quality=90, subsampling=1)), WG256, 1),
           (as_440(pillow_file(P(16, 512, 512), "RGB", quality=95, subsampling=1)), WG1024, 2)]
    for group, extended in ((baseline, False), (ext, True)):
        got = huff_classes([f for f, _, _ in group], extended)
        assert got == [(c, n) for _, c, n in group]
    files = [f for f, _, _ in baseline + ext]
    ref = [pillow_rgb(f) for f in files]
    for serial in (False, True):
        if serial:
            monkeypatch.setenv("IMGXF_JPEG_SERIAL_HUFFMAN", "1")
        frames = jpeg_decode.decode(files, device, extended=True)
        for i, (t, r) in enumerate(zip(frames, ref)):
            assert np.array_equal(t.cpu().numpy(), r), (serial, i)


def test_mixed_batch_order_sizes_statuses_and_damage(device):
    from imagetransformations_amd import jpeg_decode
    from imagetransformations_amd._ffi import ImgxfError
    img = photo_like(3, 40, 56)
    base = pillow_file(img, "RGB", quality=80)
    prog = pillow_file(img, "RGB", quality=80, progressive=True)
    cmyk = pillow_file(img, "CMYK", quality=80)
    rgbc = pillow_file(img, "RGB", quality=80, keep_rgb=True)
    rng = np.random.default_rng(2)
    f440 = W.random_file(rng, SAMPLINGS["440"], 56, 40, jfif=True)
    other = W.random_file(rng, SAMPLINGS["411"], 33, 17)
    refused = refusal_cases()[0][0]
    files = [cmyk, base, prog, refused, f440, rgbc, other, base]
    st = []
    frames = jpeg_decode.decode(files, device, progressive=True, extended=True, statuses=st)
    assert st == [0, 0, 0, R.E_FRACTIONAL, 0, 0, 0, 0]
    assert frames[3] is None
    for i, (data, t) in enumerate(zip(files, frames)):
        if i != 3:
            assert np.array_equal(t.cpu().numpy(), pillow_rgb(data)), i
    same = [frames[i] for i in (0, 1, 2, 4, 5, 7)]                # one [6, 40, 56, 3] block, frames in input order
    assert len({t.untyped_storage().data_ptr() for t in same}) == 1
    assert [t.data_ptr() for t in same] == sorted(t.data_ptr() for t in same)
    # without `statuses` the first refused file raises; without `extended` the CMYK file is refused as before
    with pytest.raises(jpeg_decode.UnsupportedJpeg, match="file 3"):
        jpeg_decode.decode(files, device, progressive=True, extended=True)
    with pytest.raises(jpeg_decode.UnsupportedJpeg, match="file 0"):
        jpeg_decode.decode(files, device, progressive=True)
    # damaged entropy-coded data of an extended file: ImgxfError, or DAMAGED with `statuses`; never pixels
    big = large_files()[1]
    g = bytearray(big)
    sos = g.index(b"\xff\xda")
    g[sos + 40:len(g) - 2] = b"\xff\xd0" * ((len(g) - 2 - sos - 40) // 2) + b"\x00" * ((len(g) - 2 - sos - 40) % 2)
    with pytest.raises(ImgxfError):
        jpeg_decode.decode([base, bytes(g)], device, extended=True)
    trunc = big[:len(big) // 2]
    with pytest.raises((ImgxfError, jpeg_decode.UnsupportedJpeg)):
        jpeg_decode.decode([trunc], device, extended=True)
    st = []
    frames = jpeg_decode.decode([bytes(g), cmyk, trunc], device, extended=True, statuses=st)
    assert frames[0] is None and frames[2] is None and st[0] == jpeg_decode.DAMAGED and st[2] != 0 and st[1] == 0
    assert np.array_equal(frames[1].cpu().numpy(), pillow_rgb(cmyk))


def test_random_byte_damage_never_faults(device):
    from imagetransformations_amd import jpeg_decode
    from imagetransformations_amd._ffi import ImgxfError
    rng = np.random.default_rng(5)
    for f in large_files():
        for _ in range(4):
            g = bytearray(f)
            for _ in range(3):
                g[int(rng.integers(len(f) // 4, len(f) - 4))] = int(rng.integers(0, 256))
            try:
                jpeg_decode.decode([bytes(g)], device, extended=True)
            except (ImgxfError, jpeg_decode.UnsupportedJpeg):
                pass
    f = large_files()[0]
    assert np.array_equal(jpeg_decode.decode([f], device, extended=True)[0].cpu().numpy(), pillow_rgb(f))


def test_rgb_coded_baseline_file_raises_by_default(device):
    from imagetransformations_amd import jpeg_decode
    rgbc = pillow_file(photo_like(6, 40, 56), "RGB", quality=90, keep_rgb=True)
    with pytest.raises(jpeg_decode.UnsupportedJpeg, match="YCbCr"):
        jpeg_decode.decode([rgbc], device)
    assert np.array_equal(jpeg_decode.decode([rgbc], device, extended=True)[0].cpu().numpy(), pillow_rgb(rgbc))


_CHILD = r"""
import json, random, sys
import numpy as np
sys.path.insert(0, sys.argv[1])
from imagetransformations_amd import io_pipeline as IO
random.seed(9); np.random.seed(9)
n = IO.run_directory(sys.argv[2], sys.argv[3], chunk_images=4, workers=2, decoder=sys.argv[4], encoder="pillow")
print(json.dumps(dict(n=n, stats=IO.DECODE_STATS, extended=IO.EXTENDED_ON_DEVICE)))
"""


def test_run_directory_with_extended_on_device(tmp_path):
    import json
    src = tmp_path / "in"
    rng = np.random.default_rng(8)
    files = {"a/cmyk.JPEG": pillow_file(photo_like(1, 40, 56), "CMYK", quality=90),
             "a/rgb.JPEG": pillow_file(photo_like(2, 32, 48), "RGB", quality=90, keep_rgb=True),
             "a/base.JPEG": pillow_file(photo_like(3, 40, 56), "RGB", quality=90),
             "b/f440.JPEG": W.random_file(rng, SAMPLINGS["440"], 37, 29, jfif=True),
             "b/ycck.JPEG": ycck(pillow_file(photo_like(4, 33, 21), "CMYK", quality=85)),
             "b/frac.JPEG": refusal_cases()[0][0],                # Pillow rejects it too: skipped, uncounted
             "b/base2.JPEG": pillow_file(photo_like(5, 48, 64), "RGB", quality=75)}
    for name, data in files.items():
        (src / os.path.dirname(name)).mkdir(parents=True, exist_ok=True)
        (src / name).write_bytes(data)
    outs = {}
    for decoder, ext in (("pillow", "0"), ("device", "1"), ("device", "0")):
        dst = tmp_path / f"{decoder}{ext}"
        env = dict(os.environ, IMGXF_JPEG_EXTENDED=ext)
        r = subprocess.run([sys.executable, "-c", _CHILD, ROOT, str(src), str(dst), decoder], env=env, capture_output=True, text=True,
                           timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        res = json.loads(r.stdout.strip().splitlines()[-1])
        assert res["n"] == 6 * 8 and res["extended"] == (ext == "1")
        if decoder == "device":
            assert res["stats"] == ({"device": 6, "pillow": 0} if ext == "1" else {"device": 2, "pillow": 4})
        outs[decoder + ext] = {f: (dst / f).read_bytes() for f in sorted(os.listdir(dst))}
    assert outs["pillow0"] == outs["device1"] == outs["device0"]
