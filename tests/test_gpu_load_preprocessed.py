"""GPU: io_pipeline.load_preprocessed — from a directory of JPEG files to the model input in one call: threaded reads, the
device reader (Pillow for the files it refuses), tensor_maps.preprocess_list — against Image.open(p).convert("RGB") and
the Pillow + CPU torch preprocessing, exactly."""
import os

import numpy as np
import pytest
import torch
from PIL import Image

from preprocess_list_ref import MEAN, STD, pillow_ref

pytestmark = pytest.mark.gpu


def _smooth(rng, h, w, c=3):
    """A seeded smooth image: a coarse random grid upsampled, plus a little noise."""
    coarse = rng.integers(0, 256, (max(2, h // 32 + 2), max(2, w // 32 + 2), c), dtype=np.uint8)
    img = Image.fromarray(coarse.squeeze() if c == 1 else coarse).resize((w, h), Image.BICUBIC)
    a = np.asarray(img).astype(np.int16) + rng.integers(-6, 7, (h, w) if c == 1 else (h, w, c))
    return np.clip(a, 0, 255).astype(np.uint8)


def test_directory_to_model_input(device, tmp_path, capsys):
    from imagetransformations_amd import io_pipeline
    rng = np.random.default_rng(11)
    sizes = [(375, 500), (500, 375), (333, 500), (256, 256), (480, 640), (213, 320), (300, 451), (97, 131)]
    sub = tmp_path / "n01" / "deep"
    sub.mkdir(parents=True)
    for i, (h, w) in enumerate(sizes):
        Image.fromarray(_smooth(rng, h, w)).save(str((tmp_path if i % 2 else sub) / f"img_{i:02d}.JPEG"), quality=(75, 90)[i % 2])
    Image.fromarray(_smooth(rng, 360, 480)).save(str(tmp_path / "progressive.jpeg"), quality=90, progressive=True)
    Image.fromarray(_smooth(rng, 280, 410, 1)).save(str(sub / "gray.jpeg"), quality=75)
    (tmp_path / "garbage.jpeg").write_bytes(bytes(rng.integers(0, 256, 4096, dtype=np.uint8)))
    (tmp_path / "notes.txt").write_text("not an image")
    paths = io_pipeline.list_images(str(tmp_path))
    assert len(paths) == len(sizes) + 3
    opened = []
    for p in paths:
        try:
            opened.append((p, np.asarray(Image.open(p).convert("RGB"))))
        except Exception:
            pass
    assert len(opened) == len(sizes) + 2
    for mean, std in ((None, None), (MEAN, STD)):
        got, kept = io_pipeline.load_preprocessed(paths, 256, 224, mean, std)
        assert kept == [p for p, _ in opened]
        assert got.shape == (len(opened), 3, 224, 224) and got.is_cuda
        for i, (p, a) in enumerate(opened):
            assert torch.equal(got[i].cpu(), pillow_ref(a, 256, 224, mean, std)), os.path.basename(p)
    assert "Failed to load image" in capsys.readouterr().out and "garbage.jpeg" not in "".join(kept)
    got, kept = io_pipeline.load_preprocessed([], 256, 224)
    assert got.shape == (0, 3, 224, 224) and kept == []
