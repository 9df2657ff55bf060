"""The engine under the batched drivers: "a list of images, N transformations each" becomes one upload per image size, one
launch per group of images that drew the same thing, and results copied back through a bounded window of pinned memory.
It knows no transformation by name: the caller draws the plans, says how entries group and in which order the groups of
one size run, and supplies the launch (`run_group`)."""
from __future__ import annotations

import numpy as np
import torch
from PIL import Image

from . import ops, staging


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
    negative and passes the budget by at most one group's result."""

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

    def collect(self) -> None:
        """Wait for the oldest copy and build its PIL images."""
        dl, entries, rgbx = self.pending.pop(0)
        host = dl.numpy()
        for j, (_, i, k) in enumerate(entries):
            self.results[i][k] = staging.image_from_rgbx(host[j]) if rgbx else Image.fromarray(host[j])
        self.nbytes -= host.nbytes


def run_grouped(images, plans, dev, run_group, key=lambda transform_type, args: (transform_type, args), order=None,
                other=None, sink=None, tee=False):
    """images[i]: a PIL image or an [H, W, 3] uint8 device frame (never copied to the host); plans[i]: the
    [(type, args, file name)] its caller drew for it.  Returns results[i][k], the image of plans[i][k].

    Every 8-bit RGB image is uploaded once, with the others of its size.  Entries of one size with the same
    `key(type, args)` (a (type, args) pair of its own) form a group, which goes through
    `run_group(type, args, batch, entries)`: batch [B, H, W, 3] holds the frames of entries [(row, i, k)] in that order,
    the result is a [B, ...] device tensor — or None: the group leaves its images as they are, and the results are the
    input objects themselves.  The groups of one size run in the order their keys first came up, or sorted (stably) by
    `order(key)`.  `sink(out, names)`, when given, consumes a group's result on the device with its file names instead
    of it being copied back (those results stay None) — with `tee` the images come back as well.  An image that is not
    8-bit RGB is the caller's: results[i] = other(i)."""
    results = [[None] * len(p) for p in plans]
    by_size = {}
    for i, img in enumerate(images):
        if is_rgb(img):
            by_size.setdefault(size_of(img), []).append(i)
        else:
            results[i] = other(i)
    back = CopyBack(results)
    for members in by_size.values():
        if all(isinstance(images[i], torch.Tensor) for i in members):               # already on the device (JPEG reader)
            frames = torch.stack([images[i] for i in members])
        else:
            frames = staging.upload([np.asarray(images[i].cpu() if isinstance(images[i], torch.Tensor) else images[i])
                                     for i in members], dev)                        # one pinned block, async H2D
        groups = {}
        for row, i in enumerate(members):
            for k, (transform_type, args, _) in enumerate(plans[i]):
                groups.setdefault(key(transform_type, args), []).append((row, i, k))
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
    while back.pending:
        back.collect()
    return results
