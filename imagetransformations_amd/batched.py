"""The engine under the batched drivers: "a list of images, N transformations each" becomes one upload per image size, one
launch per group of images that drew the same thing, and results copied back through a bounded window of pinned memory.
It knows no transformation by name: the caller draws the plans, says how entries group and in which order the groups of
one size run, and supplies the launch (`run_group`)."""
from __future__ import annotations

import numpy as np
import torch
from PIL import Image

from . import ops, staging


# Pixels per row when a list call's output block is handled as one RGB image (CopyBack.add_block).  driver_list sizes its
# allocation from this constant, and its outputs start on whole pixels (multiples of 48 bytes: tests/test_driver_list_host.py).
BLOCK_ROW = 16384


def size_of(img):
    """(width, height) of a PIL image or of an [H, W, 3] device frame (the device JPEG reader's output)."""
    return (int(img.shape[1]), int(img.shape[0])) if isinstance(img, torch.Tensor) else img.size


def is_rgb(img) -> bool:
    return (img.dim() == 3 and img.shape[-1] == 3 and img.dtype == torch.uint8) if isinstance(img, torch.Tensor) else img.mode == 'RGB'


class CopyBack:
    """Results on their way back to the host.  `add` queues a group's copy and returns at once, so the caller keeps
    launching: the host waits per result only when it builds the images.  The window of copies in flight is bounded
    (staging.PENDING_BUDGET bytes of pinned memory): beyond it the oldest results are turned into images before the next
    group is queued.  `nbytes` counts what was handed to staging.download and has not been collected: it is never
    negative and passes the budget by at most one group's result — or by one list call's block (`add_block`), which goes
    back whole: as RGBX it is 4/3 of the call's outputs (about 1.2 GB of pinned memory for a chunk of 256 photographs,
    more for a caller that hands the driver more frames at once), the budget cannot split it, it stays alive as long as
    any PIL image built from it does, and `zero_copy_reserve` counts its frames, not the padding between them."""

    def __init__(self, results):
        self.results, self.pending, self.nbytes = results, [], 0       # pending: (Download, entries, frames are RGBX)

    def add(self, out: torch.Tensor, entries) -> None:
        # RGB frames go back as RGBX and become PIL images that share the pinned block (staging.image_from_rgbx)
        rgbx = out.dim() == 4 and out.shape[-1] == 3 and out.dtype == torch.uint8 and \
            staging.zero_copy_reserve(out.shape[0] * out.shape[1] * out.shape[2] * 4)
        if rgbx:
            out = ops.permute_channels(out, (0, 1, 2, 2))
        self.pending.append((staging.download(out), entries, rgbx))
        self.nbytes += out.numel() * out.element_size()
        while self.nbytes > staging.PENDING_BUDGET and len(self.pending) > 1:
            self.collect()

    def add_block(self, block: torch.Tensor, pieces) -> None:
        """Queue ONE copy of a list call's flat output block; pieces: [(byte offset, (h, w), i, k)] of the RGB frames in it.
        A block that is a whole number of rows of BLOCK_ROW pixels, with its frames on pixel boundaries, is expanded to
        RGBX as one image in one launch, and the PIL images share the pinned block as `add`'s do."""
        rows = block.numel() // (3 * BLOCK_ROW)
        rgbx = block.numel() == rows * 3 * BLOCK_ROW and 0 < rows <= 32767 and all(p[0] % 3 == 0 for p in pieces) and \
            staging.zero_copy_reserve(sum(h * w * 4 for _, (h, w), _, _ in pieces))
        if rgbx:
            block = ops.permute_channels(block.view(1, rows, BLOCK_ROW, 3), (0, 1, 2, 2))
        self.pending.append((staging.download(block), pieces, "block4" if rgbx else "block"))
        self.nbytes += block.numel()
        while self.nbytes > staging.PENDING_BUDGET and len(self.pending) > 1:
            self.collect()

    def collect(self) -> None:
        """Wait for the oldest copy and build its PIL images."""
        dl, entries, rgbx = self.pending.pop(0)
        host = dl.numpy()
        if rgbx == "block4":
            flat = host.reshape(-1, 4)
            for off, (h, w), i, k in entries:
                self.results[i][k] = staging.image_from_rgbx(flat[off // 3:off // 3 + h * w].reshape(h, w, 4))
        elif rgbx == "block":
            for off, (h, w), i, k in entries:
                self.results[i][k] = Image.fromarray(host[off:off + h * w * 3].reshape(h, w, 3))
        else:
            for j, (_, i, k) in enumerate(entries):
                self.results[i][k] = staging.image_from_rgbx(host[j]) if rgbx else Image.fromarray(host[j])
        self.nbytes -= host.nbytes


def run_grouped(images, plans, dev, run_group, key=lambda transform_type, args: (transform_type, args), order=None,
                other=None, sink=None, tee=False, list_route=None):
    """images[i]: a PIL image or an [H, W, 3] uint8 device frame (never copied to the host); plans[i]: the
    [(type, args, file name)] its caller drew for it.  Returns results[i][k], the image of plans[i][k].

    Every 8-bit RGB image is uploaded once, with the others of its size.  Entries of one size with the same
    `key(type, args)` (a (type, args) pair of its own) form a group, which goes through
    `run_group(type, args, batch, entries)`: batch [B, H, W, 3] holds the frames of entries [(row, i, k)] in that order,
    the result is a [B, ...] device tensor — or None: the group leaves its images as they are, and the results are the
    input objects themselves.  The groups of one size run in the order their keys first came up, or sorted (stably) by
    `order(key)`.  `sink(out, names)`, when given, consumes a group's result on the device with its file names instead
    of it being copied back (those results stay None) — with `tee` the images come back as well.  An image that is not
    8-bit RGB is the caller's: results[i] = other(i).

    `list_route = (phase_of, run_list)`, when given, takes entries out of the groups: `phase_of(type, args)` is None for
    an entry that stays grouped, or the number of the list call it joins.  After the grouped entries of all sizes, each
    phase in ascending order goes through ONE `run_list(phase, frames, items)` call — frames: the [H, W, 3] device
    frames of all images, items: [(frame index, type, args, i, k)] — which returns (block, outputs, refused): the flat
    uint8 allocation that holds the outputs, outputs[j] an [H', W', 3] view into it, and the indices of the items it did
    not take.  Those run as groups, as above.  The sink receives a list output as a [1, H', W', 3] view; what is copied
    back goes in one copy of the block."""
    results = [[None] * len(p) for p in plans]
    by_size = {}
    for i, img in enumerate(images):
        if is_rgb(img):
            by_size.setdefault(size_of(img), []).append(i)
        else:
            results[i] = other(i)
    back = CopyBack(results)

    def run_groups(frames, groups):
        ordered = groups.items() if order is None else sorted(groups.items(), key=lambda g: order(g[0]))
        for (transform_type, args), entries in ordered:
            batch = frames.index_select(0, torch.tensor([e[0] for e in entries], device=dev))
            out = run_group(transform_type, args, batch, entries)
            if out is None:
                for _, i, k in entries:
                    results[i][k] = images[i]
                continue
            if sink is not None:
                sink(out, [plans[i][k][2] for _, i, k in entries])
                if not tee:
                    continue
            back.add(out, entries)

    listed = {}                                     # phase -> [(size, row, i, k)]
    held = {}                                       # size -> its frames, kept for the list calls
    for size, members in by_size.items():
        if all(isinstance(images[i], torch.Tensor) for i in members):               # already on the device (JPEG reader)
            frames = torch.stack([images[i] for i in members]) if list_route is None else None
        else:
            frames = staging.upload([np.asarray(images[i].cpu() if isinstance(images[i], torch.Tensor) else images[i])
                                     for i in members], dev)                        # one pinned block, async H2D
        groups = {}
        for row, i in enumerate(members):
            for k, (transform_type, args, _) in enumerate(plans[i]):
                phase = None if list_route is None else list_route[0](transform_type, args)
                if phase is None:
                    groups.setdefault(key(transform_type, args), []).append((row, i, k))
                else:
                    listed.setdefault(phase, []).append((size, row, i, k))
        if list_route is not None:
            if frames is None:                      # device frames are read in place by the list calls
                frames = _Rows([images[i] for i in members])
            held[size] = frames
        if groups:
            run_groups(frames.stacked() if isinstance(frames, _Rows) else frames, groups)
    for phase in sorted(listed):
        todo = listed[phase]
        frame_of, flat = {}, []
        for size, row, i, k in todo:
            if i not in frame_of:
                frame_of[i] = len(flat)
                flat.append(held[size][row])
        block, outputs, refused = list_route[1](phase, flat, [(frame_of[i], plans[i][k][0], plans[i][k][1], i, k)
                                                              for _, _, i, k in todo])
        pieces = []
        for j, (size, row, i, k) in enumerate(todo):
            out = outputs[j]
            if out is None:
                continue
            if sink is not None:
                sink(out[None], [plans[i][k][2]])
                if not tee:
                    continue
            pieces.append((out.storage_offset() - block.storage_offset(), (out.shape[0], out.shape[1]), i, k))
        if pieces:
            back.add_block(block, pieces)
        again = {}                                  # size -> groups of the entries the list call refused
        for j in refused:
            size, row, i, k = todo[j]
            again.setdefault(size, {}).setdefault(key(plans[i][k][0], plans[i][k][1]), []).append((row, i, k))
        for size, groups in again.items():
            frames = held[size]
            run_groups(frames.stacked() if isinstance(frames, _Rows) else frames, groups)
    while back.pending:
        back.collect()
    return results


class _Rows:
    """The device frames of one size, as they came: indexed in place by the list calls, stacked (once) only when a group
    of that size needs a batch."""

    def __init__(self, frames):
        self.frames, self._stacked = frames, None

    def __getitem__(self, row):
        return self.frames[row]

    def stacked(self) -> torch.Tensor:
        if self._stacked is None:
            self._stacked = torch.stack(self.frames)
        return self._stacked
