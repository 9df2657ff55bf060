"""The on-disk steps either side of the hot path (/root/reference/transformation.py:73-89 load,
:159-162 save) as a streaming pipeline around the batched driver: JPEG decode and encode stay on
the CPU with Pillow — the same codec the reference uses, so the pixels entering and leaving are the
reference's — but run in worker threads (Pillow releases the GIL inside the codecs) that overlap
with the GPU work of the neighbouring chunks (`encoder="device"` moves the encode of RGB → *.jpg outputs
to the GPU writer, `jpeg.encode`, whose files are byte-identical to Pillow's):

    decode chunk k+1  |  transform chunk k on the GPU  |  encode + write chunk k-1

Chunks are consecutive slices of the file list in the reference's order, and the batched driver
draws per image in list order, so the `random` / `np.random` streams — hence file names and pixels
— are those of the reference's one-image-at-a-time loop."""
from __future__ import annotations

import os
from concurrent.futures import ThreadPoolExecutor
from typing import Callable, Iterable, List, Sequence, Tuple

from PIL import Image


def list_images(data_path: str, suffix: str = ".jpeg") -> List[str]:
    """The file order of the reference's load_data (:74-78): os.walk order, *.jpeg, case-insensitive."""
    paths = []
    for root, _, files in os.walk(data_path):
        paths.extend(os.path.join(root, f) for f in files if f.lower().endswith(suffix))
    return paths


def _decode(path: str):
    try:
        return Image.open(path).convert("RGB"), path          # :83
    except Exception as e:                                     # the reference guards only the loading (:85-86)
        print(f"Failed to load image {path}: {e}")
        return None


def _read(path: str):
    try:
        with open(path, "rb") as f:
            return f.read(), path
    except Exception as e:
        print(f"Failed to load image {path}: {e}")
        return None


DECODE_STATS = {"device": 0, "pillow": 0}      # files decoded by the device reader / handed to Pillow by decoder="device"
PROGRESSIVE_ON_DEVICE = os.environ.get("IMGXF_JPEG_PROGRESSIVE") == "1"   # progressive files on the device reader too (opt-in)
EXTENDED_ON_DEVICE = os.environ.get("IMGXF_JPEG_EXTENDED") == "1"         # CMYK / YCCK / RGB-coded / odd sampling too (opt-in)


def _decode_on_device(read):
    """[(bytes, path)] -> [(frame, path)]: one `jpeg_decode.decode` over the chunk; a file outside the device reader's
    class (progressive unless PROGRESSIVE_ON_DEVICE, CMYK unless EXTENDED_ON_DEVICE, ...) or one it finds damaged comes
    back as None and is decoded by Pillow, as :83 does, and uploaded — counted in DECODE_STATS so that the share is
    visible.  Only those files leave the batch."""
    import io
    import numpy as np
    import torch
    from . import jpeg_decode
    from ._ffi import ImgxfError
    items = [r for r in read if r is not None]
    try:
        frames = jpeg_decode.decode([d for d, _ in items], progressive=PROGRESSIVE_ON_DEVICE, extended=EXTENDED_ON_DEVICE,
                                    statuses=[])
    except (jpeg_decode.UnsupportedJpeg, ImgxfError):           # (not a per-file verdict: the whole chunk goes to Pillow)
        frames = [None] * len(items)
    out = []
    for t, (d, p) in zip(frames, items):
        if t is not None:
            out.append((t, p))
            DECODE_STATS["device"] += 1
            continue
        try:
            img = Image.open(io.BytesIO(d)).convert("RGB")
            out.append((torch.from_numpy(np.asarray(img)).cuda(), p))
            DECODE_STATS["pillow"] += 1
        except Exception as e:
            print(f"Failed to load image {p}: {e}")
    return out


def load_preprocessed(paths: Sequence[str], resize: int = 256, crop: int = 224, mean=None, std=None, workers: int = 8,
                      interpolation="bilinear"):
    """From file names to a model input in one call: the files are read on a thread pool, decoded on the device as one
    chunk (`_decode_on_device`: a file the device reader refuses or finds damaged goes to Pillow, one Pillow cannot open
    is skipped with the reference's message) and preprocessed by `tensor_maps.preprocess_list` in one launch.
    `interpolation`: Resize's filter as `tensor_maps.resample_filter` reads it (default BILINEAR), checked before any file
    is read.
    Returns (float32 [N, 3, crop, crop], the paths of the N files kept, in order)."""
    from . import tensor_maps
    filt = tensor_maps.resample_filter(interpolation)
    with ThreadPoolExecutor(max_workers=workers) as pool:
        read = list(pool.map(_read, paths))
    items = _decode_on_device(read)
    return (tensor_maps.preprocess_list([t for t, _ in items], resize, crop, mean, std, interpolation=filt),
            [p for _, p in items])


def load_random_resized_crops(paths: Sequence[str], size=224, scale=(0.08, 1.0), ratio=(3.0 / 4.0, 4.0 / 3.0), flip_p=0.5,
                              mean=None, std=None, workers: int = 8, interpolation="bilinear"):
    """`load_preprocessed`'s training-time twin: the files are read on a thread pool and decoded on the device as one
    chunk, one box and one flip per kept file are drawn by `tensor_maps.random_resized_crop_params` (torch's default CPU
    generator, consumed as Compose([RandomResizedCrop(size, scale, ratio), RandomHorizontalFlip(flip_p)]) does image by
    image), and `tensor_maps.resized_crop_list` makes the batch in one launch.  `interpolation`: RandomResizedCrop's
    filter as `tensor_maps.resample_filter` reads it (default BILINEAR), checked before any file is read.
    Returns (float32 [N, 3, Sh, Sw], the paths of the N files kept, in order)."""
    from . import tensor_maps
    filt = tensor_maps.resample_filter(interpolation)
    with ThreadPoolExecutor(max_workers=workers) as pool:
        read = list(pool.map(_read, paths))
    items = _decode_on_device(read)
    frames = [t for t, _ in items]
    boxes, flips = tensor_maps.random_resized_crop_params([(t.shape[0], t.shape[1]) for t in frames], scale, ratio, flip_p)
    return (tensor_maps.resized_crop_list(frames, boxes, size, flips, mean=mean, std=std, interpolation=filt),
            [p for _, p in items])


def resize_files(paths: Sequence[str], out_dir: str, size, interpolation="bicubic", quality: int = 75, workers: int = 8, *,
                 subsampling=-1, optimize: bool = False, progressive: bool = False):
    """Shrink (or enlarge) JPEG files without the pixels ever visiting the host: the files are read on a thread pool and
    decoded on the device as one chunk (`_decode_on_device`: a file the device reader refuses goes to Pillow, one Pillow
    cannot open is skipped with the reference's message), resized by `resize_list.resize_list` in one launch, written
    by `jpeg.encode_list_views` and stored under their own names in `out_dir`.  `size`: an int for torchvision
    `Resize(int)`'s shorter-side rule, or one (width, height) pair for every file.  Each stage is bit-exact, so file k is
    byte for byte `Image.open(p).convert("RGB").resize(size_k, interpolation).save(..., "JPEG", quality=quality,
    subsampling=subsampling, optimize=optimize, progressive=progressive)` (Pillow's spellings; the defaults are Pillow's
    default file), every class in one list call of the writer (progressive files: from
    `jpeg.PROGRESSIVE_LIST_MIN_SHAPES` distinct sizes on).  `interpolation`, `subsampling` and `progressive` (a bool) are
    checked before any file is read.  Returns the output paths of the files kept, in order."""
    from . import jpeg, resize_list, tensor_maps
    filt = tensor_maps.resample_filter(interpolation)
    jpeg.sampling(subsampling, 3)
    if not isinstance(progressive, bool):
        raise ValueError(f"progressive must be True or False, not {progressive!r}")
    os.makedirs(out_dir, exist_ok=True)
    with ThreadPoolExecutor(max_workers=workers) as pool:
        items = _decode_on_device(list(pool.map(_read, paths)))
        frames = [t for t, _ in items]
        if isinstance(size, int):
            sizes = resize_list.shorter_side_sizes([(t.shape[0], t.shape[1]) for t in frames], size)
        else:
            sizes = [tuple(size)] * len(frames)
        files = jpeg.encode_list_views(resize_list.resize_list(frames, sizes, filt), quality, subsampling=subsampling,
                                       optimize=optimize, progressive=progressive)
        outs = [os.path.join(out_dir, os.path.basename(p)) for _, p in items]
        list(pool.map(_write, files, outs))
    return outs


def _chunks(seq: Sequence, n: int) -> Iterable[Sequence]:
    for i in range(0, len(seq), n):
        yield seq[i:i + n]


def run_directory(data_path: str, out_dir: str, chunk_images: int = 256, workers: int = 8,
                  transform: Callable[[List[Tuple[Image.Image, str]]], List[Tuple[str, Image.Image]]] | None = None,
                  encoder: str = "device", decoder: str | None = None) -> int:
    """load_data + apply_all_transformations + save over a directory, streamed.  `transform` maps a
    chunk [(image, path)] to [(file name, image)] in output order; default: the batched
    eight-transformation driver.  Returns the number of files written.  Both on-disk steps default to the device since
    round 3 (files byte-identical to Pillow's, pixels identical to Pillow's; "pillow" selects the host libraries the
    reference uses; with a caller's own `transform` the decoder defaults to "pillow", since it receives PIL images).  `decoder="device"`: worker threads only READ the
    files; the chunk is decoded by the GPU reader (`jpeg_decode.decode`, pixels identical to Pillow's) and the frames
    go to the batched driver without ever visiting the host."""
    if decoder is None:                                         # a caller's own `transform` is written against PIL images
        decoder = "device" if transform is None else "pillow"
    device_driver = transform is None and encoder == "device"
    if transform is None:
        from .transformation import apply_all_transformations_batched_named as transform
        from .transformation import apply_all_transformations_batched_to_files as to_files
    if encoder not in ("pillow", "device"):
        raise ValueError("encoder must be 'pillow' or 'device'")
    if decoder not in ("pillow", "device"):
        raise ValueError("decoder must be 'pillow' or 'device'")
    load = _read if decoder == "device" else _decode
    os.makedirs(out_dir, exist_ok=True)
    chunk_paths = list(_chunks(list_images(data_path), chunk_images))
    written = 0
    with ThreadPoolExecutor(max_workers=workers) as pool:
        decoding = pool.map(load, chunk_paths[0]) if chunk_paths else None
        saving = []
        for k in range(len(chunk_paths)):
            chunk = [d for d in decoding if d is not None]
            if k + 1 < len(chunk_paths):                        # the next chunk decodes (is read) while this one is on the GPU
                decoding = pool.map(load, chunk_paths[k + 1])
            if decoder == "device":
                chunk = _decode_on_device(chunk)
            if device_driver:                                   # transforms + JPEG writer, nothing but the files comes back
                for fut in saving:
                    fut.result()
                saving = []
                written += len(to_files(chunk, out_dir)) if chunk else 0
                continue
            named = transform(chunk) if chunk else []
            if decoder == "device":                             # (apply_blur's radius-0 pass-through hands a device frame back)
                named = [(nm, Image.fromarray(im.cpu().numpy()) if hasattr(im, "cpu") else im) for nm, im in named]
            for fut in saving:                                  # chunk k-1 has been encoding meanwhile
                fut.result()
            written += len(named)
            saving = []
            if encoder == "device":
                named = _save_on_device(named, out_dir, pool, saving)
            saving += [pool.submit(_save, img, os.path.join(out_dir, name)) for name, img in named]
        for fut in saving:
            fut.result()
    return written


def _save(img: Image.Image, path: str) -> None:
    img.save(path)                                              # Image.save defaults, as :162


def _write(data: bytes, path: str) -> None:
    with open(path, "wb") as f:
        f.write(data)


def _save_on_device(named, out_dir: str, pool, saving: list):
    """Encode the RGB images bound for *.jpg / *.jpeg files with the GPU writer (the files are Pillow's, byte for byte:
    tests/test_gpu_jpeg.py): all of them, whatever their sizes, go into ONE pinned block, cross PCIe in one copy and are
    encoded as views of it by one `jpeg.encode_list_views` call (one size only: the batch writer, as
    transformation._encode_held).  Queues the writes on `pool`; returns what is left for Pillow (other modes / formats,
    images carrying a comment Pillow would embed)."""
    import numpy as np
    import torch
    from . import _list_block, jpeg
    items, rest = [], []
    for name, img in named:
        if img.mode == "RGB" and name.lower().endswith((".jpg", ".jpeg")) and "comment" not in img.info and min(img.size) > 0:
            items.append((name, np.asarray(img)))
        else:
            rest.append((name, img))
    if not items:
        return rest
    offs, total = _list_block.slots([a.size for _, a in items])  # 16-byte aligned frames: the transform's wide loads
    offs = offs.tolist()
    block = _list_block.pack_pinned(total, zip(offs, (a for _, a in items))).cuda(non_blocking=True)
    shapes = {a.shape for _, a in items}
    if len(shapes) == 1:
        h, w, _ = items[0][1].shape
        files = jpeg.encode_views(torch.as_strided(block, (len(items), h, w, 3), (_list_block.r16(3 * h * w), 3 * w, 3, 1)))
    else:
        files = jpeg.encode_list_views(_list_block.hwc_views(block, offs, [a.shape[:2] for _, a in items]))
    for (name, _), data in zip(items, files):
        saving.append(pool.submit(_write, data, os.path.join(out_dir, name)))
    return rest


SEVERITY_INDICES = [0, 1001, 2002, 3003, 4004, 10000, 10001, 12002, 13003, 14004, 15005, 20000, 22002, 23003,
                    24004, 25005, 30000, 40000]          # transformation.py:28 (zip with five labels uses the first five)
SEVERITY_LABELS = [1, 2, 3, 4, 5]


def load_data_npy(data_path: str, store_dir: str) -> int:
    """The CIFAR-10-C extraction step (transformation.py:20-71): every *.npy under `data_path`
    with shape (50000, 32, 32, 3) contributes the images at the first five severity indices,
    written as `{corruption}_severity{level}_idx{index}.png`.  The arrays are memory-mapped
    (153 MB each; five 3 KiB slices are read), the bytes written are the reference's."""
    import numpy as np
    os.makedirs(store_dir, exist_ok=True)
    npy_files = []
    for root, _, files in os.walk(data_path):
        npy_files.extend(os.path.join(root, f) for f in files if f.lower().endswith('.npy'))
    extracted_count = 0
    for file_path in npy_files:
        try:
            corruption_data = np.load(file_path, mmap_mode="r")
            corruption_name = os.path.splitext(os.path.basename(file_path))[0]
            if corruption_data.shape != (50000, 32, 32, 3):
                print(f"  Warning: Unexpected shape for {corruption_name}.npy: {corruption_data.shape}. Skipping.")
                continue
            for s_idx, severity_level in zip(SEVERITY_INDICES, SEVERITY_LABELS):
                img_array = np.array(corruption_data[s_idx])
                if img_array.dtype != np.uint8:
                    img_array = img_array.astype(np.uint8)
                Image.fromarray(img_array).save(
                    os.path.join(store_dir, f"{corruption_name}_severity{severity_level}_idx{s_idx}.png"))
                extracted_count += 1
        except Exception as e:
            print(f"Failed to process file {file_path}: {e}")
    return extracted_count
