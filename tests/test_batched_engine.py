"""CPU: the engine under the batched drivers (imagetransformations_amd.batched) with the staging copies replaced by host
stand-ins: results land where their plan entry is, groups run in the caller's order, and the window of copies back
counts what it downloads (third finding: the old loops added the RGB bytes of a group and subtracted the RGBX
bytes of its copy, so the count drifted negative by numel / 3 per group and the bound stopped holding)."""
import numpy as np
import pytest
import torch
from PIL import Image

from conftest import synth
from imagetransformations_amd import batched, ops, staging

DEV = torch.device("cpu")


class HostCopies:
    """staging.upload / staging.download / ops.permute_channels on the host, counting the bytes of copies back that have
    started and have not been collected (`numpy()` is the collection)."""

    def __init__(self, monkeypatch, zero_copy: bool):
        self.outstanding, self.peak, self.largest, self.downloads, self.uploads = 0, 0, 0, 0, 0
        monkeypatch.setattr(staging, "upload", self.upload)
        monkeypatch.setattr(staging, "download", self.download)
        monkeypatch.setattr(ops, "permute_channels", lambda t, order: t[..., list(order)].contiguous())
        monkeypatch.setattr(staging, "_zc_ok", None)                     # probe again under this budget
        monkeypatch.setattr(staging, "ZERO_COPY_BUDGET", (1 << 30) if zero_copy else 0)

    def upload(self, arrays, device):
        self.uploads += 1
        return torch.from_numpy(np.stack([np.asarray(a) for a in arrays]))

    def download(self, t):
        copies, nbytes = self, t.numel() * t.element_size()
        self.outstanding += nbytes
        self.peak, self.largest, self.downloads = max(self.peak, self.outstanding), max(self.largest, nbytes), self.downloads + 1

        class Copy:
            def numpy(self):
                copies.outstanding -= nbytes
                return t.numpy()
        return Copy()


def plans_for(images, values):
    """Per image: 'add' with a value from `values` (keys repeat across images), 'same' (a None-returning group), 'neg'."""
    return [[("add", (values[i % len(values)],), f"img{i}_add.jpg"), ("same", (), f"img{i}_same.jpg"), ("neg", (), f"img{i}_neg.jpg")]
            for i in range(len(images))]


def run_group(transform_type, args, batch, entries):
    assert batch.shape[0] == len(entries)
    if transform_type == "add":
        return batch + args[0]                                           # uint8, wraps
    if transform_type == "neg":
        return 255 - batch
    return None


def expected(a, transform_type, args):
    return (a + np.uint8(args[0])) if transform_type == "add" else 255 - a


@pytest.mark.parametrize("zero_copy", [True, False])
def test_results_land_at_their_plan_entries(monkeypatch, zero_copy):
    copies = HostCopies(monkeypatch, zero_copy)
    sizes = [(8, 8), (5, 7), (8, 8), (8, 8), (5, 7), (6, 6), (8, 8)]
    arrays = [synth(400 + i, *hw) for i, hw in enumerate(sizes)]
    images = [Image.fromarray(a) for a in arrays]
    plans = plans_for(images, [3, 9])
    results = batched.run_grouped(images, plans, DEV, run_group)
    assert copies.uploads == 3 and copies.outstanding == 0               # one upload per size
    # (8, 8): add 3 (images 0, 2, 6), add 9 (3), neg; (5, 7): add 9 (1), add 3 (4), neg; (6, 6): add 9, neg
    assert copies.downloads == 8
    for i, plan in enumerate(plans):
        for k, (transform_type, args, _) in enumerate(plan):
            if transform_type == "same":
                assert results[i][k] is images[i]                        # the input object itself
            else:
                got = results[i][k]
                assert got.mode == "RGB" and got.size == images[i].size and got.readonly == int(zero_copy)
                assert np.array_equal(np.asarray(got), expected(arrays[i], transform_type, args)), (i, k)


def test_tensor_frames_are_stacked_not_uploaded_and_other_images_go_to_the_caller(monkeypatch):
    copies = HostCopies(monkeypatch, True)
    arrays = [synth(420 + i, 6, 9) for i in range(3)]
    images = [torch.from_numpy(a) for a in arrays] + [Image.fromarray(synth(430, 6, 9, 1))]
    plans = plans_for(images, [1])
    marker = [object(), object(), object()]
    results = batched.run_grouped(images, plans, DEV, run_group, other=lambda i: marker if i == 3 else None)
    assert copies.uploads == 0 and results[3] is marker
    for i in range(3):
        assert results[i][1] is images[i]
        assert np.array_equal(np.asarray(results[i][2]), 255 - arrays[i])
    with pytest.raises(KeyError):                                        # what the caller's callback raises comes through
        batched.run_grouped(images, plans, DEV, run_group, other=lambda i: {}[i])


def test_groups_of_one_size_run_in_the_callers_order(monkeypatch):
    HostCopies(monkeypatch, True)
    images = [Image.fromarray(synth(440 + i, *hw)) for i, hw in enumerate([(4, 4), (4, 4), (3, 5), (4, 4)])]
    plans = plans_for(images, [7, 2, 7])
    ran = []

    def recording(transform_type, args, batch, entries):
        ran.append((tuple(batch.shape[1:3]), transform_type, args, [(i, k) for _, i, k in entries]))
        return run_group(transform_type, args, batch, entries)

    batched.run_grouped(images, plans, DEV, recording)                   # the order the keys first come up, size by size
    assert ran == [((4, 4), "add", (7,), [(0, 0), (3, 0)]), ((4, 4), "same", (), [(0, 1), (1, 1), (3, 1)]),
                   ((4, 4), "neg", (), [(0, 2), (1, 2), (3, 2)]), ((4, 4), "add", (2,), [(1, 0)]),
                   ((3, 5), "add", (7,), [(2, 0)]), ((3, 5), "same", (), [(2, 1)]), ((3, 5), "neg", (), [(2, 2)])]
    ran.clear()
    batched.run_grouped(images, plans, DEV, recording, order=lambda key: key[0] == "add")      # stable: 'add' groups last
    assert [(r[0], r[1], r[2]) for r in ran] == [((4, 4), "same", ()), ((4, 4), "neg", ()), ((4, 4), "add", (7,)), ((4, 4), "add", (2,)),
                                                 ((3, 5), "same", ()), ((3, 5), "neg", ()), ((3, 5), "add", (7,))]
    ran.clear()

    def by_type(transform_type, args, batch, entries):
        ran.append((tuple(batch.shape[1:3]), transform_type, args, [(i, k) for _, i, k in entries]))

    batched.run_grouped(images, plans, DEV, by_type, key=lambda t, args: (t, ()))              # grouped by type alone
    assert ran[0] == ((4, 4), "add", (), [(0, 0), (1, 0), (3, 0)]) and len(ran) == 6


def test_sink_takes_the_results_on_the_device(monkeypatch):
    copies = HostCopies(monkeypatch, True)
    arrays = [synth(450 + i, 4, 6) for i in range(3)]
    images = [Image.fromarray(a) for a in arrays]
    plans = plans_for(images, [5])
    sunk = {}

    def sink(out, names):
        assert isinstance(out, torch.Tensor) and out.shape[0] == len(names)
        sunk.update(zip(names, out.numpy()))

    results = batched.run_grouped(images, plans, DEV, run_group, sink=sink)
    assert copies.downloads == 0 and sorted(sunk) == sorted(n for p in plans for t, _, n in p if t != "same")
    assert all(results[i][k] is (images[i] if k == 1 else None) for i in range(3) for k in range(3))
    assert np.array_equal(sunk["img2_neg.jpg"], 255 - arrays[2])
    results = batched.run_grouped(images, plans, DEV, run_group, sink=sink, tee=True)
    assert copies.downloads == 2 and np.array_equal(np.asarray(results[1][0]), arrays[1] + np.uint8(5))


@pytest.mark.parametrize("zero_copy", [True, False])
def test_copies_in_flight_stay_within_the_budget(monkeypatch, zero_copy):
    """PENDING_BUDGET worth a few results: the bytes of copies started and not collected pass it by at most one result,
    the engine's own count is that figure at every step, and both end at zero."""
    copies = HostCopies(monkeypatch, zero_copy)
    windows = []

    class Watched(batched.CopyBack):
        def __init__(self, results):
            super().__init__(results)
            windows.append(self)

        def add(self, out, entries):
            super().add(out, entries)
            assert self.nbytes == copies.outstanding >= 0
            assert self.nbytes <= staging.PENDING_BUDGET or len(self.pending) == 1

        def collect(self):
            super().collect()
            assert self.nbytes == copies.outstanding >= 0

    monkeypatch.setattr(batched, "CopyBack", Watched)
    h, w, n = 16, 12, 60
    arrays = [synth(500 + i, h, w) for i in range(n)]
    images = [Image.fromarray(a) for a in arrays]
    plans = plans_for(images, list(range(20)))                           # 20 'add' groups of 3 frames, one 'neg' group of 60
    budget = 4 * 3 * h * w * 3 + 1                                       # four three-frame RGB results and a byte
    monkeypatch.setattr(staging, "PENDING_BUDGET", budget)

    def watching(transform_type, args, batch, entries):
        assert windows[-1].nbytes == copies.outstanding
        return run_group(transform_type, args, batch, entries)

    results = batched.run_grouped(images, plans, DEV, watching)
    assert len(windows) == 1 and windows[0].nbytes == 0 and copies.outstanding == 0 and not windows[0].pending
    assert copies.downloads == 21
    assert copies.largest == n * h * w * (4 if zero_copy else 3)         # the RGBX tensor is what is copied and counted
    assert budget < copies.peak <= budget + copies.largest
    for i in range(n):
        assert np.array_equal(np.asarray(results[i][0]), arrays[i] + np.uint8(i % 20))
        assert np.array_equal(np.asarray(results[i][2]), 255 - arrays[i])
