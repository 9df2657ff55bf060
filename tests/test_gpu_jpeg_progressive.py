"""GPU: progressive JPEG files on the device reader (`jpeg_decode.decode(..., progressive=True)`: the layout of
imgxf_jpeg_layout_progressive_host + imgxf_jpeg_decode_progressive, then the baseline reader's IDCT and colour kernels)
against Pillow / libjpeg-turbo: bit-identical pixels, in one batch and one file at a time; mixed batches in input order;
refusals and damaged files raise as `decode` does; io_pipeline with PROGRESSIVE_ON_DEVICE."""
import glob
import io
import os
import random

import numpy as np
import pytest
from PIL import Image

from conftest import synth
from jpeg_transcode import baseline_to_progressive
from oracle import jpeg_progressive_oracle as P
from test_jpeg_decode_oracle import photo_like, pillow_rgb
from test_jpeg_progressive_oracle import _scripts, prog_bytes, refusal_cases

pytestmark = pytest.mark.gpu
REF = sorted(glob.glob(os.path.join(os.path.dirname(__file__), "golden", "reference_outputs", "*.JPEG")))


def corpus():
    """Pillow-written progressive files of every size class / sampling / quality / restart kind, the reference's files re-saved
    progressive, and transcoded scripts Pillow does not write."""
    files = []
    for h, w in [(1, 1), (7, 5), (8, 8), (16, 16), (17, 33), (31, 15), (48, 64), (100, 75), (375, 500)]:
        for sub in (0, 1, 2, "gray"):
            for q in (5, 75, 100) if h < 300 else (75,):
                img = photo_like(h * 7 + w, h, w)
                if sub == "gray":
                    buf = io.BytesIO(); Image.fromarray(img).convert("L").save(buf, "JPEG", progressive=True, quality=q); files.append(buf.getvalue())
                else:
                    files.append(prog_bytes(img, quality=q, subsampling=sub))
    img = photo_like(21, 61, 83)
    files += [prog_bytes(img, restart_marker_rows=1), prog_bytes(img, restart_marker_blocks=7, subsampling=0)]
    files += [prog_bytes(np.asarray(Image.open(p).convert("RGB")), quality=75) for p in REF[::3]]
    for kind, sub in (("color", 2), ("color", 1), ("gray", None)):
        buf = io.BytesIO()
        im = Image.fromarray(photo_like(11, 37, 53))
        (im.convert("L").save(buf, "JPEG", quality=80) if sub is None else im.save(buf, "JPEG", quality=80, subsampling=sub))
        ncomp = 1 if sub is None else 3
        for name, sc in _scripts(ncomp).items():
            files.append(baseline_to_progressive(buf.getvalue(), sc))
        files.append(baseline_to_progressive(buf.getvalue(), _scripts(ncomp)["approx"], restart_interval=3))
    return files


def test_progressive_files_in_one_batch_and_one_at_a_time(device):
    from imagetransformations_amd import jpeg_decode
    files = corpus()
    frames = jpeg_decode.decode(files, device, progressive=True)
    for i, (data, t) in enumerate(zip(files, frames)):
        assert np.array_equal(t.cpu().numpy(), pillow_rgb(data)), i
    for i in range(0, len(files), 7):
        assert np.array_equal(jpeg_decode.decode([files[i]], device, progressive=True)[0].cpu().numpy(), pillow_rgb(files[i])), i
    assert np.array_equal(frames[5].cpu().numpy(), P.decode_progressive(files[5]))


def test_full_hd_and_4k_progressive(device):
    from imagetransformations_amd import jpeg_decode
    files = [prog_bytes(photo_like(9, 1080, 1920)), prog_bytes(photo_like(10, 2160, 3840), restart_marker_rows=1)]
    for data, t in zip(files, jpeg_decode.decode(files, device, progressive=True)):
        assert np.array_equal(t.cpu().numpy(), pillow_rgb(data))


def test_mixed_batch_keeps_input_order_and_shares_blocks(device):
    from imagetransformations_amd import jpeg_decode
    img = photo_like(3, 40, 56)
    buf = io.BytesIO(); Image.fromarray(img).save(buf, "JPEG", quality=80); base = buf.getvalue()
    files = [prog_bytes(img), base, prog_bytes(img, subsampling=0), prog_bytes(photo_like(4, 33, 17)), base,
             prog_bytes(img, restart_marker_rows=1)]
    frames = jpeg_decode.decode(files, device, progressive=True)
    for data, t in zip(files, frames):
        assert np.array_equal(t.cpu().numpy(), pillow_rgb(data))
    same = [frames[i] for i in (0, 1, 2, 4, 5)]                   # one [5, 40, 56, 3] block, frames in input order
    assert len({t.untyped_storage().data_ptr() for t in same}) == 1
    assert [t.data_ptr() for t in same] == sorted(t.data_ptr() for t in same)
    # without the flag the batch is refused exactly as before (the first progressive file)
    with pytest.raises(jpeg_decode.UnsupportedJpeg, match="file 0"):
        jpeg_decode.decode(files, device)


def test_refused_and_damaged_files_raise_as_decode_does(device):
    from imagetransformations_amd import jpeg_decode
    from imagetransformations_amd._ffi import ImgxfError
    good, cases = refusal_cases()
    for data, code in cases:
        exc = ImgxfError if code == P.E_TRUNCATED else jpeg_decode.UnsupportedJpeg
        with pytest.raises(exc, match="file 1"):
            jpeg_decode.decode([good, data], device, progressive=True)
    # damaged entropy-coded data (deterministic byte flips inside scans): frames or ImgxfError, never a fault; the
    # good file decodes afterwards
    rng = np.random.default_rng(5)
    seeds = [prog_bytes(photo_like(7, 64, 96), quality=85), prog_bytes(photo_like(8, 64, 96), restart_marker_rows=1)]
    for f in seeds:
        for _ in range(6):
            g = bytearray(f)
            for _ in range(3):
                g[int(rng.integers(len(f) // 4, len(f) - 4))] = int(rng.integers(0, 256))
            try:
                jpeg_decode.decode([bytes(g)], device, progressive=True)
            except (ImgxfError, jpeg_decode.UnsupportedJpeg):
                pass
    assert np.array_equal(jpeg_decode.decode([good], device, progressive=True)[0].cpu().numpy(), pillow_rgb(good))


def test_run_directory_with_progressive_on_device(device, tmp_path, monkeypatch):
    from imagetransformations_amd import io_pipeline as IO
    src = str(tmp_path / "in")
    for i in range(6):
        d = os.path.join(src, f"n{i % 2:02d}")
        os.makedirs(d, exist_ok=True)
        Image.fromarray(synth(i, *[(32, 32), (48, 64), (37, 61)][i % 3])).save(os.path.join(d, f"img_{i}.JPEG"), quality=95)
    Image.fromarray(synth(77, 40, 56)).save(os.path.join(src, "n01", "prog.jpeg"), progressive=True, quality=80)
    outs = {}
    for name, kw, on in (("pillow", dict(decoder="pillow", encoder="pillow"), False), ("device", dict(decoder="device", encoder="pillow"), True)):
        monkeypatch.setattr(IO, "PROGRESSIVE_ON_DEVICE", on)
        dst = str(tmp_path / name)
        random.seed(9); np.random.seed(9)
        IO.DECODE_STATS.update(device=0, pillow=0)
        assert IO.run_directory(src, dst, chunk_images=4, workers=2, **kw) == 7 * 8
        if on:
            assert IO.DECODE_STATS == {"device": 7, "pillow": 0}
        outs[name] = {f: open(os.path.join(dst, f), "rb").read() for f in sorted(os.listdir(dst))}
    assert outs["pillow"] == outs["device"]
