"""The extra transformations of the reference's later variant
(/root/reference/fall_2025/transformations_code:39-52) on the HIP kernels, same names and
argument meaning.  Its `apply_*` functions are the same bodies as `transformation.py`'s and are
re-exported from there.  `apply_perspective_warp` (:54-66) wraps torchvision's
RandomPerspective on a float tensor; torchvision is not installed, so the host side restates
its parameter draws and coefficient solve on torch's own RNG / lstsq (same generator stream,
same values) and the kernel restates `_perspective_grid` + `grid_sample`, checked bit-for-bit
against those torch CPU primitives (tests/test_oracle_vs_libs.py)."""
from __future__ import annotations

import os
import random

import numpy as np
import torch
from PIL import Image

from . import batched, numpy_stream, ops, staging
from . import transformation as T
from ._perspective import _perspective_coeffs, _perspective_endpoints  # noqa: F401  (shared with transform_list)
from .transformation import (_download, _upload, apply_blur, apply_brightness, apply_contrast,  # noqa: F401
                             apply_gaussian_noise, apply_rotation, apply_scale, apply_shear,
                             apply_translation)


def vert_flip(img: Image.Image) -> Image.Image:
    """`img.transpose(Image.FLIP_LEFT_RIGHT)` (:39-41; the reference's name notwithstanding,
    it mirrors left-right)."""
    return _download(ops.flip(_upload(img)))


def rand_crop(img: Image.Image) -> Image.Image:
    """Random crop with 0.78 scale factor, resized to 32x32 with Image.resize's default
    BICUBIC filter (:43-48).  The corner comes from np.random, as in the reference."""
    w, h = img.size
    cs = int(0.78 * w)
    x, y = np.random.randint(0, w - cs + 1), np.random.randint(0, h - cs + 1)
    t = ops.crop(_upload(img), (x, y, x + cs, y + cs))
    return _download(ops.resize(t, (32, 32), ops.RESAMPLE_BICUBIC))


def apply_random_zoom(img: Image.Image, scale_factor: float) -> Image.Image:
    """Zoom transformation (1.0 to 1.1 range) = apply_scale (:50-52)."""
    return apply_scale(img, scale_factor)


def draw_perspective_coeffs(width: int, height: int, distortion_scale: float):
    """The random part of RandomPerspective(distortion_scale, p=1.0).forward on torch's global
    generator: the `torch.rand(1) < p` draw first (always true for p = 1), then get_params."""
    torch.rand(1)
    return _perspective_coeffs(*_perspective_endpoints(width, height, distortion_scale))


def apply_perspective_warp(img: Image.Image, distortion_scale: float = 0.2) -> Image.Image:
    """Symmetric perspective warp (:54-66): ToTensor -> RandomPerspective(distortion_scale,
    p=1.0) -> ToPILImage.  Seed with torch.manual_seed, as for the reference."""
    w, h = img.size
    coeffs = draw_perspective_coeffs(w, h, distortion_scale)
    return _download(ops.perspective(_upload(img), coeffs))


output_dir = None       # the reference hard-codes a directory (:16); None = do not save

TRANSFORMATIONS_2D = {
    'scale': {'min': 0.9, 'max': 1.4, 'step': 0.1},
    'rotation': {'min': -22.5, 'max': 22.5, 'step': 2.5},
    'lighten_darken': {'min': -0.05, 'max': 0.05, 'step': 0.01},
    'gaussian_noise': {'min': 0.0, 'max': 0.1, 'step': 0.01},
    'translation': {'min': -50, 'max': 50, 'step': 5},
    'contrast': {'min': 0, 'max': 1, 'step': 0.1},
    'blur': {'min': 0, 'max': 5, 'step': 0.5},
    'shear': {'min': 0, 'max': 1, 'step': 0.1},
    'vert_flip': {'apply': True},
    'rand_crop': {'apply': True},
    'zoom': {'min': 1.0, 'max': 1.1, 'step': 0.01},
    'perspective_warp': {'min': 0.0, 'max': 0.2, 'step': 0.05},
}

_DISPATCH = {
    'scale': apply_scale, 'rotation': apply_rotation, 'lighten_darken': apply_brightness,
    'gaussian_noise': apply_gaussian_noise, 'contrast': apply_contrast, 'shear': apply_shear,
    'blur': apply_blur, 'zoom': apply_random_zoom, 'perspective_warp': apply_perspective_warp,
    'translation': apply_translation, 'vert_flip': vert_flip,
}


def apply_all_transformations(images):
    """The twelve-transformation driver of the later variant (:68-155): images = [(PIL image,
    name)]; per image and per type one `random.choice` over the value grid (two for the
    translation, none for the flip and the crop), file names `{name}_{type}_{value}_corrupted.jpg`."""
    transformed_images = []
    total_transforms = 0
    for i, (img, name) in enumerate(images):
        ext = '.jpg'
        for transform_type, params in TRANSFORMATIONS_2D.items():
            if transform_type in ('vert_flip', 'rand_crop'):
                new_filename = f"{name}_{transform_type}_corrupted{ext}"
                transformed_img = vert_flip(img) if transform_type == 'vert_flip' else rand_crop(img)
            else:
                possible_values = T.grid_values(params)
                if transform_type == 'translation':
                    tx = random.choice(possible_values)
                    ty = random.choice(possible_values)
                    new_filename = f"{name}_{transform_type}_{tx}_{ty}_corrupted{ext}"
                    transformed_img = apply_translation(img, tx, ty)
                else:
                    transform_value = random.choice(possible_values)
                    new_filename = f"{name}_{transform_type}_{transform_value}_corrupted{ext}"
                    transformed_img = _DISPATCH[transform_type](img, transform_value)
            if output_dir is not None:
                transformed_img.save(os.path.join(output_dir, new_filename))
            transformed_images.append(transformed_img)
            total_transforms += 1
        if (i + 1) % 1000 == 0:
            print(f"Processed {i + 1}/{len(images)} original images, created {total_transforms} transformed images")
    return transformed_images


def apply_all_transformations_batched(images):
    """`apply_all_transformations` with the work grouped for the GPU: the same `random`,
    `np.random` and `torch` draws in the same order, the same file names and the same pixels in
    the same output order — but every image is uploaded once and all RGB images of one size that
    drew the same (type, value) go through one batched launch (perspective warps and crops of one
    size share a launch with per-frame coefficients / windows).  images: [(PIL image, name)].

    With `transformation.DRIVER_LIST` ("1", or "auto" when the RGB images hold more than one size) every type of ALL sizes runs
    in ONE `driver_list.apply_list` call — one copy of one block, at most three launches plus one per distinct blur
    radius, no resample plan — instead of one launch per (size, type, value); entries that call refuses (float blurs
    that another kernel family serves among them), radius-0 blurs and images that are not 8-bit RGB go where they go
    without it."""
    if T.DRIVER_LIST not in ("auto", "0", "1"):
        raise ValueError(f'DRIVER_LIST / IMGXF_DRIVER_LIST must be "auto", "0" or "1", got {T.DRIVER_LIST!r}')
    dev = T._device()
    # ---- draws, image by image, in the order the per-image loop makes them.  The np.random calls (the noise's normals, the
    # crop's two randints) are only listed here, in that order: nothing else uses np.random, so one pass over its stream on
    # the device serves them all afterwards (T._numpy_mixed), or the host makes them one by one
    plans, extra = [], {}
    np_requests, np_slots = [], []                      # request -> where its result goes: (key of extra, None | 0 | 1, shape)
    for i, (img, name) in enumerate(images):
        w, h = img.size
        plan = []
        for transform_type, params in TRANSFORMATIONS_2D.items():
            if transform_type == 'vert_flip':
                plan.append((transform_type, (), f"{name}_{transform_type}_corrupted.jpg"))
            elif transform_type == 'rand_crop':
                cs = int(0.78 * w)
                extra[(i, len(plan))] = [None, None, cs]
                np_requests += [("randint", 0, w - cs + 1), ("randint", 0, h - cs + 1)]
                np_slots += [((i, len(plan)), 0, None), ((i, len(plan)), 1, None)]
                plan.append((transform_type, (), f"{name}_{transform_type}_corrupted.jpg"))
            else:
                possible_values = T.grid_values(params)
                if transform_type == 'translation':
                    tx, ty = random.choice(possible_values), random.choice(possible_values)
                    plan.append((transform_type, (tx, ty), f"{name}_{transform_type}_{tx}_{ty}_corrupted.jpg"))
                    continue
                value = random.choice(possible_values)
                if transform_type == 'gaussian_noise':
                    shape = np.array(img).shape
                    np_requests.append(("normal", int(np.prod(shape)), value * 255))
                    np_slots.append(((i, len(plan)), None, shape))
                elif transform_type == 'perspective_warp':
                    extra[(i, len(plan))] = draw_perspective_coeffs(w, h, value)
                plan.append((transform_type, (value,), f"{name}_{transform_type}_{value}_corrupted.jpg"))
        plans.append(plan)
    drawn = T._numpy_mixed(np_requests, dev)
    if drawn is None:
        drawn = numpy_stream.host_mixed(np_requests)
    for v, (key, slot, shape) in zip(drawn, np_slots):
        if slot is None:
            extra[key] = v.reshape(shape)               # float32 noise: a device tensor, or the host's array
        else:
            extra[key][slot] = v

    def noise_on_device(i, k):
        z = extra[(i, k)]
        return z if isinstance(z, torch.Tensor) else torch.from_numpy(z).to(dev)

    def crop(t, i, k):
        x, y, cs = (int(v) for v in extra[(i, k)])
        return ops.crop(t, (x, y, x + cs, y + cs))

    def per_image(i):                                   # not 8-bit RGB, rare: the per-image bodies, with the draws made above
        img, out = images[i][0], []
        for k, (transform_type, args, _) in enumerate(plans[i]):
            if transform_type == 'gaussian_noise':
                out.append(_download(ops.add_noise(_upload(img), noise_on_device(i, k))))
            elif transform_type == 'perspective_warp':
                out.append(_download(ops.perspective(_upload(img), extra[(i, k)])))
            elif transform_type == 'rand_crop':
                out.append(_download(ops.resize(crop(_upload(img), i, k), (32, 32), ops.RESAMPLE_BICUBIC)))
            else:
                out.append(_DISPATCH[transform_type](img, *args))
        return out

    def run_group(transform_type, args, batch, entries):
        if transform_type == 'blur':
            return T._blur_group(batch, args[0])
        if transform_type == 'gaussian_noise':
            zs = [extra[(i, k)] for _, i, k in entries]
            return ops.add_noise(batch, torch.stack(zs) if isinstance(zs[0], torch.Tensor) else staging.upload(zs, dev))
        if transform_type == 'perspective_warp':
            return ops.perspective(batch, [extra[(i, k)] for _, i, k in entries])
        if transform_type == 'rand_crop':               # crops differ per image but share their size: gather them, then one resize launch
            crops = torch.stack([crop(batch[j], i, k) for j, (_, i, k) in enumerate(entries)])
            return ops.resize(crops, (32, 32), ops.RESAMPLE_BICUBIC)
        if transform_type == 'vert_flip':
            return ops.flip(batch)
        return T._TENSOR_FNS['scale' if transform_type == 'zoom' else transform_type](batch, *args)

    # Frames of different sizes (DRIVER_LIST): everything but the radius-0 blur (the input object itself) leaves the groups
    # and runs in one list call for the whole chunk; the float blurs that call refuses (another kernel family serves them:
    # 16-byte rows, by and large) come back as groups.  One phase: every np.random number has been drawn above.
    def run_list(phase, frames, items):
        from . import driver_list
        entries = []
        for f, transform_type, args, i, k in items:
            if transform_type == 'gaussian_noise':
                z = extra[(i, k)]
                args = (z if isinstance(z, torch.Tensor) else staging.upload(z, dev),)
            elif transform_type == 'perspective_warp':
                args = (extra[(i, k)],)
            elif transform_type == 'rand_crop':
                args = tuple(int(v) for v in extra[(i, k)][:2])
            entries.append((f, transform_type, args))
        return driver_list.apply_list_block(frames, entries)

    sizes = {batched.size_of(img) for img, _ in images if batched.is_rgb(img)}
    use_list = T.DRIVER_LIST == "1" or (T.DRIVER_LIST == "auto" and len(sizes) > 1)
    # perspective warps and crops of one size share a launch whatever they drew (per-frame coefficients / windows)
    results = batched.run_grouped([img for img, _ in images], plans, dev, run_group, other=per_image,
                                  key=lambda t, args: (t, () if t in ('perspective_warp', 'rand_crop') else args),
                                  list_route=(lambda t, args: None if t == 'blur' and T._blur_ksize(args[0]) == 0 else 0,
                                              run_list) if use_list else None)
    transformed_images = []
    for i, plan in enumerate(plans):
        for k, (_, _, new_filename) in enumerate(plan):
            if output_dir is not None:
                results[i][k].save(os.path.join(output_dir, new_filename))
            transformed_images.append(results[i][k])
    return transformed_images
