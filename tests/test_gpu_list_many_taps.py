"""GPU: output rows with more than 64 vertical taps in the list kernels that read their tables from the block
(tensor_maps.preprocess_list, driver_list.apply_list's scale), against Pillow / the oracle, exact.  The band engine's row
loop keeps a row's first 64 coefficients one per lane and reads the rest from the table; the sizes here are the smallest
that put 70 to 97 taps on a row and still run in the kernels (asserted: no entry may take another route)."""
import numpy as np
import pytest
import torch

from oracle import imgxf_oracle as O
from preprocess_list_ref import MEAN, STD, noise_frames, pillow_ref

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("norm", [False, True])
@pytest.mark.parametrize("crop", [4, 3])                         # 3: the scalar store path
def test_preprocess_list_rows_with_more_than_64_taps(device, crop, norm):
    from imagetransformations_amd import tensor_maps as tm
    sizes, resize = [(140, 140), (150, 141), (141, 150)], 4
    block = tm.preprocess_layout(tm.preprocess_geometry(sizes, resize, crop), crop)
    hd, rec, units = tm.preprocess_block_views(block)
    assert np.all(rec["unit_rows"] == crop) and len(units) == len(sizes) and hd["lds_bytes"] < 6 * 1024
    taps = [int(block.view(np.int32)[int(r["bounds_y"]) + 1:int(r["bounds_y"]) + 2 * crop:2].max()) for r in rec]
    assert min(taps) >= 70                                       # every frame has rows past the 64 lanes' coefficients
    frames = noise_frames(sizes, seed=11)
    dev = [torch.from_numpy(a).to(device) for a in frames]
    mean, std = (MEAN, STD) if norm else (None, None)
    got = tm.preprocess_list(dev, resize, crop, mean, std).cpu()
    assert got.shape == (len(frames), 3, crop, crop)
    for i, a in enumerate(frames):
        assert torch.equal(got[i], pillow_ref(a, resize, crop, mean, std)), (i, a.shape, crop)


def test_driver_list_scale_rows_with_more_than_64_taps(device):
    """Factor 0.05: 3 x 3 and 4 x 3 windows of 70 and 97 Lanczos taps per row, pasted on the black canvas; beside a
    factor 1 entry in the same launch."""
    from imagetransformations_amd import driver_list as dl
    sizes = [(70, 70), (97, 70)]
    frames = noise_frames(sizes, seed=12)
    dev = [torch.from_numpy(a).to(device) for a in frames]
    entries = [(0, 'scale', (0.05,)), (1, 'scale', (0.05,)), (0, 'scale', (1.0,))]
    geometry = [(i, dl.TYPES[name], *sizes[i], 3) for i, name, _ in entries]
    lay = dl.layout(geometry, [dl.entry_params(name, args) for _, name, args in entries])
    hd, rec, _ = dl.block_views(lay["block"])
    assert rec["unit_rows"].tolist() == [3, 4, 16] and np.all(lay["status"] == dl.OK) and hd["lds_bytes"] < 6 * 1024
    words = lay["block"].view(np.int32)
    taps = [int(words[int(r["bounds_y"]) + 1:int(r["bounds_y"]) + 2 * int(r["win_h"]):2].max()) for r in rec]
    assert taps[:2] == [70, 97]
    outputs, refused = dl.apply_list(dev, entries)
    assert refused == []
    for (i, name, args), out in zip(entries, outputs):
        want = O.apply_scale(frames[i], *args)
        assert torch.equal(out.cpu(), torch.from_numpy(np.ascontiguousarray(want))), (sizes[i], args)
