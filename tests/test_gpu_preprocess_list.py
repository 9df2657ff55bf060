"""GPU: tensor_maps.preprocess_list — Resize + CenterCrop + ToTensor + Normalize of a list of frames of different sizes in
one launch — against Pillow + CPU torch (exact), over the size list and (resize, crop) pairs of preprocess_list_ref."""
import numpy as np
import pytest
import torch

from preprocess_list_ref import MEAN, PAIRS, SIZES, STD, noise_frames, pillow_ref, workload_sizes

pytestmark = pytest.mark.gpu


def _tm():
    from imagetransformations_amd import tensor_maps
    return tensor_maps


def _check(got, frames, resize, crop, mean=None, std=None, what=""):
    got = got.cpu()
    assert got.shape == (len(frames), 3, crop, crop) and got.dtype == torch.float32
    for i, a in enumerate(frames):
        assert torch.equal(got[i], pillow_ref(a, resize, crop, mean, std)), (what, i, a.shape, resize, crop)


@pytest.mark.parametrize("norm", [False, True])
@pytest.mark.parametrize("resize,crop", PAIRS)
def test_size_list_in_one_call_equals_pillow(device, resize, crop, norm):
    frames = noise_frames()
    dev = [torch.from_numpy(a).to(device) for a in frames]
    mean, std = (MEAN, STD) if norm else (None, None)
    _check(_tm().preprocess_list(dev, resize, crop, mean, std), frames, resize, crop, mean, std)


@pytest.mark.parametrize("resize,crop", [(256, 224), (40, 32)])
def test_frames_cut_from_one_flat_allocation(device, resize, crop):
    """As jpeg_decode.decode lays frames out: consecutive byte offsets, so bases fall on every residue modulo 16."""
    sizes = [(37, 61), (7, 3), (255, 257), (1, 1), (257, 255), (1, 9), (333, 500), (32, 32), (375, 500), (213, 320),
             (3, 700), (500, 333), (334, 500), (300, 256), (224, 224), (256, 341), (500, 375), (5000, 257), (640, 480)]
    frames = noise_frames(sizes, seed=2)
    want = torch.stack([pillow_ref(a, resize, crop, MEAN, STD) for a in frames])
    residues = [set() for _ in frames]
    for lead in range(16):
        flat = torch.from_numpy(np.concatenate([np.zeros(lead, np.uint8)] + [a.reshape(-1) for a in frames])).to(device)
        views, pos = [], lead
        for i, a in enumerate(frames):
            views.append(flat[pos:pos + a.size].view(a.shape))
            residues[i].add(views[-1].data_ptr() % 16)
            pos += a.size
        assert torch.equal(_tm().preprocess_list(views, resize, crop, MEAN, STD).cpu(), want), lead
    assert all(len(r) == 16 for r in residues)


def test_column_windows_of_wider_tensors(device):
    """Row stride > 3 W, first byte at any offset inside the row."""
    rng = np.random.default_rng(3)
    frames, views = [], []
    for (h, w), x0, extra in (((375, 500), 1, 7), ((300, 256), 5, 1), ((64, 47), 2, 3), ((500, 375), 3, 125), ((1, 9), 4, 4)):
        wide = rng.integers(0, 256, (h, x0 + w + extra, 3), dtype=np.uint8)
        frames.append(np.ascontiguousarray(wide[:, x0:x0 + w]))
        views.append(torch.from_numpy(wide).to(device)[:, x0:x0 + w])
        assert h == 1 or views[-1].stride(0) > 3 * w
    _check(_tm().preprocess_list(views, 256, 224), frames, 256, 224)
    _check(_tm().preprocess_list(views, 40, 32, MEAN, STD), frames, 40, 32, MEAN, STD)


def test_order_shuffled_with_duplicates(device):
    frames = noise_frames(SIZES[:9] + SIZES[23:], seed=4)
    dev = [torch.from_numpy(a).to(device) for a in frames]
    base = _tm().preprocess_list(dev, 256, 224, MEAN, STD)
    order = np.random.default_rng(5).integers(0, len(dev), 40).tolist()
    assert len(set(order)) < len(order)
    got = _tm().preprocess_list([dev[i] for i in order], 256, 224, MEAN, STD)
    assert torch.equal(got, base[order])
    _check(got, [frames[i] for i in order], 256, 224, MEAN, STD)


def test_single_frame_out_slice_and_guards(device):
    tm = _tm()
    frames = noise_frames([(375, 500), (500, 333), (224, 224)], seed=6)
    dev = [torch.from_numpy(a).to(device) for a in frames]
    _check(tm.preprocess_list(dev[:1], 256, 224, MEAN, STD), frames[:1], 256, 224, MEAN, STD)      # N = 1
    big = torch.full((7, 3, 224, 224), -7.25, dtype=torch.float32, device=device)                   # out= a slice of a batch
    ret = tm.preprocess_list(dev, 256, 224, out=big[2:5])
    assert ret.data_ptr() == big[2:5].data_ptr() and ret.shape == (3, 3, 224, 224)
    _check(big[2:5], frames, 256, 224)
    assert bool((big[:2] == -7.25).all()) and bool((big[5:] == -7.25).all())
    for crop, resize in ((224, 256), (31, 40)):                                                      # guard floats round a plain out
        n, guard = len(dev), 1024
        flat = torch.full((2 * guard + n * 3 * crop * crop,), 123.5, dtype=torch.float32, device=device)
        out = flat[guard:-guard].view(n, 3, crop, crop)
        tm.preprocess_list(dev, resize, crop, MEAN, STD, out=out)
        _check(out, frames, resize, crop, MEAN, STD)
        assert bool((flat[:guard] == 123.5).all()) and bool((flat[-guard:] == 123.5).all())


def test_odd_crops_take_the_scalar_store_path(device):
    frames = noise_frames([(375, 500), (37, 61), (500, 375), (1, 1)], seed=7)
    dev = [torch.from_numpy(a).to(device) for a in frames]
    for resize, crop in ((256, 223), (256, 1), (50, 50), (33, 30), (300, 299)):
        _check(_tm().preprocess_list(dev, resize, crop, MEAN, STD), frames, resize, crop, MEAN, STD)


def test_workload_of_1024_frames_equals_preprocess(device):
    tm = _tm()
    sizes = workload_sizes()
    assert len(set(sizes)) == 343 and sizes.count((375, 500)) == 193 and sizes.count((500, 375)) == 69
    rng = np.random.default_rng(8)
    frames = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in sizes]
    dev = [torch.from_numpy(a).to(device) for a in frames]
    got = tm.preprocess_list(dev, 256, 224, MEAN, STD)
    for i, t in enumerate(dev):
        assert torch.equal(got[i], tm.preprocess(t[None], 256, 224, MEAN, STD)[0]), (i, sizes[i])
    _check(got[:32], frames[:32], 256, 224, MEAN, STD)


def test_frames_beyond_the_limit_go_through_preprocess(device, monkeypatch):
    tm = _tm()
    sizes = [(375, 500), (1080, 1920), (500, 375), (1200, 1600), (224, 224), (1080, 1920), (640, 480)]
    frames = noise_frames(sizes, seed=9)
    dev = [torch.from_numpy(a).to(device) for a in frames]
    want = tm.preprocess_list(dev, 256, 224, MEAN, STD)
    monkeypatch.setattr(tm, "PREPROCESS_LIST_LDS_BYTES", 16 * 1024)
    geo = tm.preprocess_geometry(sizes, 256, 224)
    fits = tm.preprocess_block_views(tm.preprocess_layout(geo, 224))[1]["unit_rows"] > 0
    assert fits.tolist() == [True, False, True, False, True, False, True]          # interleaved
    got = tm.preprocess_list(dev, 256, 224, MEAN, STD)
    assert torch.equal(got, want)
    _check(got, frames, 256, 224, MEAN, STD)
    monkeypatch.setattr(tm, "PREPROCESS_LIST_LDS_BYTES", 1024)                      # every frame beyond it: no launch at all
    assert torch.equal(tm.preprocess_list(dev, 256, 224, MEAN, STD), want)


def test_errors_and_the_empty_list(device):
    tm = _tm()
    ok = torch.zeros((8, 9, 3), dtype=torch.uint8, device=device)
    with pytest.raises(TypeError):
        tm.preprocess_list([ok, ok.float()])
    with pytest.raises(TypeError):
        tm.preprocess_list([ok, ok.cpu()])
    with pytest.raises(TypeError):
        tm.preprocess_list([ok, np.zeros((8, 9, 3), np.uint8)])
    for bad in (torch.zeros((8, 9), dtype=torch.uint8, device=device), torch.zeros((8, 9, 4), dtype=torch.uint8, device=device),
                torch.zeros((1, 8, 9, 3), dtype=torch.uint8, device=device), torch.zeros((0, 9, 3), dtype=torch.uint8, device=device),
                torch.zeros((8, 3, 9), dtype=torch.uint8, device=device).permute(0, 2, 1)):
        with pytest.raises(ValueError):
            tm.preprocess_list([ok, bad])
    with pytest.raises(ValueError, match="come together"):
        tm.preprocess_list([ok], mean=MEAN)
    with pytest.raises(ValueError, match="3 entries"):
        tm.preprocess_list([ok], mean=[0.5], std=[0.5])
    with pytest.raises(ValueError, match="CenterCrop larger than the resized image"):
        tm.preprocess_list([ok], 224, 256)
    for bad_out in (torch.empty((1, 3, 224, 224), dtype=torch.float64, device=device), torch.empty((2, 3, 224, 224), device=device),
                    torch.empty((1, 3, 224, 224)), torch.empty((1, 3, 224, 448), device=device)[..., ::2]):
        with pytest.raises(ValueError, match="out must be"):
            tm.preprocess_list([ok], out=bad_out)
    if torch.cuda.device_count() > 1:
        with pytest.raises(ValueError, match="one device"):
            tm.preprocess_list([ok, ok.to("cuda:1")])
    empty = tm.preprocess_list([], 256, 224)
    assert empty.shape == (0, 3, 224, 224) and empty.dtype == torch.float32
    assert empty.device == torch.device("cuda", torch.cuda.current_device())


def test_second_stream_without_device_synchronise(device):
    tm = _tm()
    frames = noise_frames(SIZES[:8], seed=10)
    dev = [torch.from_numpy(a).to(device) for a in frames]
    torch.cuda.synchronize()
    s = torch.cuda.Stream(device)
    with torch.cuda.stream(s):
        got = tm.preprocess_list(dev, 256, 224, MEAN, STD)
        total = got.sum(dim=(1, 2, 3))                       # consumed on s, nothing in between
        host = got.to("cpu", non_blocking=False)
    want = torch.stack([pillow_ref(a, 256, 224, MEAN, STD) for a in frames])
    assert torch.equal(host, want)
    s.synchronize()
    assert torch.equal(total.cpu(), want.to(device).sum(dim=(1, 2, 3)).cpu())
